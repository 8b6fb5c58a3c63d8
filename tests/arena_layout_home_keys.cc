// home_layout of csrc/dg_arena.h with the touched-keys array dg_mutate_home adds (the sixth
// per-key array, which the join leaves unused), checked on the host:
// tests/test_arena_layout_home_keys.py builds this with ASan and UBSan and runs it.  For key
// counts and tile counts around every rounding step: the measuring and the carving pass agree,
// `keys` stands where the unused array stood (no offset behind it moves), holds nk + 1 words, is 256-byte aligned, overlaps no other
// region and can be written end to end, as can every other region beside it.
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

static size_t pad(size_t b) { return (b + 255) / 256 * 256; }

static void run(u64 nk, u64 a_tiles) {
  const u64 EDIT = 1536, WORDS = 8 + 512 + 4 * 1536 + 1536 / 2 + 2048 + 2048 / 2;  // SMALL_EDIT, SMALL_WORDS
  Arena measure;
  home_layout(measure, EDIT, nk, a_tiles, WORDS);
  const size_t total = measure.bytes();
  char* blk = (char*)aligned_alloc(256, total);
  Arena real(blk);
  const HomeScratch s = home_layout(real, EDIT, nk, a_tiles, WORDS);
  CHECK(real.off == measure.off, "measured %zu, carved %zu", measure.off, real.off);
  const size_t idx = (nk + 1) * 8;
  const std::vector<Region> regs = {
      {"ed.key", s.ed.key, EDIT * 8},     {"ed.val", s.ed.val, EDIT * 8},   {"ed.ts", s.ed.ts, EDIT * 8},
      {"ed.cnt", s.ed.cnt, EDIT * 8},     {"ed.node", s.ed.node, EDIT * 4}, {"a_lo", s.idx.a_lo, idx},
      {"a_off", s.idx.a_off, idx},        {"end", s.idx.end, idx},          {"shift", s.idx.shift, idx},
      {"gap", s.idx.gap, idx},            {"keys", s.keys, idx},            {"tile_u0", s.tile_u0, (a_tiles + 2) * 8},
      {"moved", s.moved, 4},              {"res", s.res, WORDS * 8}};
  size_t end = 0;
  for (size_t i = 0; i < regs.size(); i++) {
    const Region& g = regs[i];
    CHECK(g.p != nullptr, "%s: null", g.name);
    const size_t off = (char*)g.p - blk;
    CHECK(off % 256 == 0, "%s: offset %zu not 256-byte aligned", g.name, off);
    CHECK(off == end, "%s: offset %zu, the region before it ends (padded) at %zu", g.name, off, end);
    CHECK(off + g.bytes <= total, "%s: ends at %zu of %zu", g.name, off + g.bytes, total);
    memset(g.p, 0x5a, g.bytes);  // (ASan: every byte inside the block)
    end = off + pad(g.bytes);
    g_checked++;
  }
  CHECK(end == measure.off, "the regions end at %zu, the arena at %zu", end, measure.off);
  // the size with the array unused (six per-key arrays then as now): nothing moved
  const size_t old = EDIT * 36 + 6 * pad(idx) + pad((a_tiles + 2) * 8) + 256 + pad(WORDS * 8);
  CHECK(measure.off == old, "home_layout is %zu bytes, was %zu", measure.off, old);
  // the keys follow the five index arrays directly
  CHECK((char*)s.keys == (char*)s.idx.gap + pad(idx), "keys not behind gap");
  // the mutation's ops are its key count's bound: m ops -> at most m keys fit, and one more word
  ((u64*)s.keys)[nk] = 1;
  free(blk);
}

int main() {
  const u64 SIZES[] = {0, 1, 2, 30, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024};
  for (u64 nk : SIZES)
    for (u64 a_tiles : SIZES) run(nk, a_tiles);
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
