// sdiff_layout of csrc/dg_arena.h (the streaming store diff's scratch), checked on the host:
// tests/test_arena_layout_sdiff.py builds this with ASan and UBSan and runs it.  For tile
// counts and mask sizes around every rounding step: the measuring and the carving pass
// agree, every region lies inside a block of exactly bytes(), starts 256-byte aligned with
// its size padded to 256 bytes, overlaps no other, and can be written from its first to its
// last element -- the mask through the last word the kernels may touch (the words of the
// last tile's places, which its workgroup reads unconditionally).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dg_arena.h"

using namespace dg;
typedef uint64_t u64;

static int g_fail = 0;
static long g_checked = 0;
#define CHECK(c, ...)                               \
  do {                                              \
    if (!(c)) {                                     \
      if (g_fail++ < 20) {                          \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
    }                                               \
  } while (0)

struct Region {
  const char* name;
  void* p;
  size_t bytes;
};

// restated from csrc/dg_launch.h (plain arithmetic: this file builds without HIP)
static const u64 TILE = 2048;
static u64 tiles_of(u64 na, u64 nb) { return (na + nb + TILE - 1) / TILE; }
static u64 mask_words_of(u64 na, u64 nb) { return (na + nb) / 32 + TILE / 32 + 4; }

static void run(u64 tiles, u64 words) {
  Arena measure;
  sdiff_layout(measure, tiles, words);
  const size_t total = measure.bytes();
  CHECK(total % 256 == 0 && total >= measure.off && total >= 256, "total %zu for %zu", total, measure.off);
  char* blk = (char*)aligned_alloc(256, total);
  Arena real(blk);
  const SdiffScratch s = sdiff_layout(real, tiles, words);
  CHECK(real.off == measure.off, "measured %zu, carved %zu", measure.off, real.off);
  const std::vector<Region> regs = {
      {"bounds", s.bounds, 4 * (tiles + 1) * 8}, {"cnt_k", s.cnt_k, tiles * 8}, {"cnt_r", s.cnt_r, tiles * 8},
      {"off_k", s.off_k, tiles * 8},             {"off_r", s.off_r, tiles * 8}, {"mask", s.mask, words * 4}};
  size_t end = 0;
  for (size_t i = 0; i < regs.size(); i++) {
    const Region& g = regs[i];
    CHECK(g.p != nullptr, "%s: null", g.name);
    const size_t off = (char*)g.p - blk;
    CHECK(off % 256 == 0, "%s: offset %zu not 256-byte aligned", g.name, off);
    CHECK(off == end, "%s: offset %zu, the region before it ends (padded) at %zu", g.name, off, end);
    CHECK(off + g.bytes <= total, "%s: ends at %zu of %zu", g.name, off + g.bytes, total);
    for (size_t j = 0; j < i; j++) {
      const size_t o2 = (char*)regs[j].p - blk;
      CHECK(!g.bytes || !regs[j].bytes || off + g.bytes <= o2 || o2 + regs[j].bytes <= off, "%s overlaps %s",
            g.name, regs[j].name);
    }
    if (g.bytes) memset(g.p, 0x5a, g.bytes);  // (ASan: every byte inside the block)
    end = off + (g.bytes + 255) / 256 * 256;
    g_checked++;
  }
  CHECK(end == measure.off, "the regions end at %zu, the arena at %zu", end, measure.off);
  free(blk);
}

int main() {
  const u64 ROWS[] = {0, 1, 31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 1000003};
  for (u64 na : ROWS)
    for (u64 nb : ROWS) {
      const u64 t = tiles_of(na, nb), w = mask_words_of(na, nb);
      run(t, w);
      // the last word any kernel touches: the word of the last tile's first place, plus the
      // TILE / 32 + 2 words its workgroup stages
      if (t) {
        const u64 last_p0 = na + nb;  // (an upper bound of any tile's first place)
        CHECK(last_p0 / 32 + TILE / 32 + 2 <= w, "mask of %llu words for places to %llu", (unsigned long long)w,
              (unsigned long long)last_p0);
      }
    }
  for (u64 t : {u64(0), u64(1), u64(31), u64(32), u64(33), u64(1023), u64(1024), u64(1025)})
    for (u64 w : {u64(1), u64(63), u64(64), u64(65), u64(4097)}) run(t, w);
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
