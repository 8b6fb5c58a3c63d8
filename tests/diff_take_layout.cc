// diff_take_scratch of csrc/dg_diff_scratch.h (dg_merkle_diff_take's scratch), checked on the
// host: tests/test_merkle_diff_take_abi.py builds this with ASan and UBSan and runs it.  For
// depths around the subtree size and the group size and row counts around zero: dg_merkle_diff's
// arrays sit where launch_merkle_diff puts them (its scratch does not grow and a take's keys
// read the same after either call), the two added arrays follow, every region lies inside a
// block of exactly `words` words, overlaps no other and can be written from its first to its
// last element, and the whole grows over the diff's by na + nb + 1 + tiles words, not by more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dg_diff_scratch.h"

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
  u64 off, words;
};

static void run(uint32_t depth, u64 na, u64 nb) {
  const u64 nt = diff_tiles(depth);
  const DiffTakeScratch s = diff_take_scratch(depth, na, nb);
  CHECK(s.words == diff_take_scratch_words(depth, na, nb), "two sizes");
  CHECK(s.words == diff_scratch_words(depth, na, nb) + na + nb + 1 + nt, "depth %u: grows by %llu words", depth,
        (unsigned long long)(s.words - diff_scratch_words(depth, na, nb)));
  // launch_merkle_diff's own carve, restated
  CHECK(s.bnd == 0 && s.cnt == 2 * (nt + 1) && s.keys == s.cnt + nt, "the diff's arrays moved");
  CHECK(s.loc == diff_scratch_words(depth, na, nb), "the located runs start inside the diff's scratch");
  CHECK(nt == (1ull << (depth > 12 ? depth - 12 : 0)), "depth %u: %llu subtrees", depth, (unsigned long long)nt);
  CHECK(diff_groups(depth) == (nt + 255) / 256, "groups");
  u64* blk = (u64*)malloc(s.words * sizeof(u64));
  const std::vector<Region> regs = {{"bnd", s.bnd, 2 * (nt + 1)},
                                    {"cnt", s.cnt, nt},
                                    {"keys", s.keys, na + nb},
                                    {"loc", s.loc, na + nb},
                                    {"rcnt", s.rcnt, nt}};
  for (size_t i = 0; i < regs.size(); i++) {
    const Region& g = regs[i];
    CHECK(g.off + g.words <= s.words, "%s: ends at %llu of %llu", g.name, (unsigned long long)(g.off + g.words),
          (unsigned long long)s.words);
    for (size_t j = 0; j < i; j++)
      CHECK(!g.words || !regs[j].words || g.off + g.words <= regs[j].off || regs[j].off + regs[j].words <= g.off,
            "%s overlaps %s", g.name, regs[j].name);
    if (g.words && g.off + g.words <= s.words) memset(blk + g.off, 0x5a, g.words * sizeof(u64));  // (ASan)
    g_checked++;
  }
  CHECK(regs.back().off + regs.back().words == s.words, "the last region ends the block");
  free(blk);
}

int main() {
  const u64 ROWS[] = {0, 1, 2, 255, 256, 4097, 100003};
  for (uint32_t depth : {1u, 5u, 11u, 12u, 13u, 14u, 19u, 20u, 21u, 24u})
    for (u64 na : ROWS)
      for (u64 nb : ROWS) run(depth, na, nb);
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
