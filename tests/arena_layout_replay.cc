// replay_layout of csrc/dg_arena.h (dg_replace_keysets' scratch), checked on the host:
// tests/test_arena_layout_replay.py builds this with ASan and UBSan and runs it.  For item and
// tile counts around every rounding step: the measuring and the carving pass agree, every
// region lies inside a block of exactly bytes(), starts 256-byte aligned with its size padded
// to 256 bytes, overlaps no other, and can be written from its first to its last element --
// the edit offsets through entry m (the take kernel's last tile writes key_off[n_keys], and
// the union holds at most m keys).
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

static const u64 UNION_TILE = 1024;  // csrc/dg_launch.h RP_TILE: sorted items per union workgroup

static void run(u64 m, size_t sort_bytes) {
  const u64 tiles = (m + UNION_TILE - 1) / UNION_TILE;
  Arena measure;
  replay_layout(measure, m, tiles, sort_bytes);
  const size_t total = measure.bytes();
  CHECK(total % 256 == 0 && total >= measure.off && total >= 256, "total %zu for %zu", total, measure.off);
  char* blk = (char*)aligned_alloc(256, total);
  Arena real(blk);
  const ReplayScratch s = replay_layout(real, m, tiles, sort_bytes);
  CHECK(real.off == measure.off, "measured %zu, carved %zu", measure.off, real.off);
  const std::vector<Region> regs = {{"item_lo", s.item_lo, m * 8},       {"item_len", s.item_len, m * 4},
                                    {"ukeys", s.ukeys, m * 8},           {"u_lo", s.u_lo, m * 8},
                                    {"u_len", s.u_len, m * 4},           {"e_off", s.e_off, (m + 1) * 8},
                                    {"tile_cnt", s.tile_cnt, tiles * 8}, {"tile_off", s.tile_off, tiles * 8},
                                    {"sort_tmp", s.sort_tmp, sort_bytes}};
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
  const u64 ITEMS[] = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 1000003};
  for (u64 m : ITEMS)
    for (size_t sb : {size_t(0), size_t(1), size_t(256), size_t(257), size_t(100001)}) run(m, sb);
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
