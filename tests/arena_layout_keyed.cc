// keyed_layout of csrc/dg_arena.h (dg_join_deltas_keyed's scratch), checked on the host:
// tests/test_arena_layout_keyed.py builds this with ASan and UBSan and runs it.  For delta,
// item, edit-row and tile counts around every rounding step, with and without diffs: the
// measuring and the carving pass agree, every region lies inside a block of exactly bytes(),
// starts 256-byte aligned with its size padded to 256 bytes, overlaps no other, and can be
// written from its first to its last element; the words zeroed per call are exactly the two VV
// tables, the flag and the bump pointer; the one-wait path's arrays hold m keys (the union has
// at most m) and its shift and tile_u0 their extra entries.
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

static const size_t SEG_BYTES = 16;  // csrc/dg_launch.h KsSeg: a pointer and a u64
static const size_t RUN_BYTES = 96;  // KRun: Rows (5 pointers, n), keys, n_keys, Ctx (2 pointers, n, kind)
static const u64 NODES = 1024;       // KNT
static const u64 KD_BLOCK = 256, KD_NV = 7;

static void run(u64 k, u64 m, size_t sort_bytes, u64 e_rows, u64 a_tiles, u64 uctx, bool diffs) {
  const u64 part = (m + KD_BLOCK - 1) / KD_BLOCK * KD_NV;
  Arena measure;
  keyed_layout(measure, k, SEG_BYTES, RUN_BYTES, m, sort_bytes, NODES, e_rows, part, a_tiles, uctx, diffs);
  const size_t total = measure.bytes();
  CHECK(total % 256 == 0 && total >= measure.off && total >= 256, "total %zu for %zu", total, measure.off);
  char* blk = (char*)aligned_alloc(256, total);
  Arena real(blk);
  const KeyedScratch s =
      keyed_layout(real, k, SEG_BYTES, RUN_BYTES, m, sort_bytes, NODES, e_rows, part, a_tiles, uctx, diffs);
  CHECK(real.off == measure.off, "measured %zu, carved %zu", measure.off, real.off);
  std::vector<Region> regs = {{"segs", s.segs, (k + 1) * SEG_BYTES},
                              {"runs", s.runs, k * RUN_BYTES},
                              {"cat", s.cat, m * 8},
                              {"set", s.set, m},
                              {"usorted", s.usorted, m * 8},
                              {"sort_tmp", s.sort_tmp, sort_bytes},
                              {"ukeys", s.ukeys, m * 8},
                              {"masks", s.masks, m * 8},
                              {"tabC", s.tabC, k * NODES * 8},
                              {"tabP", s.tabP, k * NODES * 8},
                              {"flag", s.flag, 4},
                              {"e_next", s.e_next, 8},
                              {"ed.key", s.ed.key, e_rows * 8},
                              {"ed.val", s.ed.val, e_rows * 8},
                              {"ed.ts", s.ed.ts, e_rows * 8},
                              {"ed.cnt", s.ed.cnt, e_rows * 8},
                              {"ed.node", s.ed.node, e_rows * 4},
                              {"a_lo", s.kd.a_lo, m * 8},
                              {"d_lo", s.kd.d_lo, m * 8},
                              {"runs_k", s.kd.runs, m * 8},
                              {"amask", s.kd.amask, m * 8},
                              {"dmask", s.kd.dmask, m * 8},
                              {"dh", s.kd.dh, m * 8},
                              {"end", s.kd.end, m * 8},
                              {"shift", s.kd.shift, (m + 1) * 8},
                              {"part", s.kd.part, part * 8},
                              {"tile_u0", s.kd.tile_u0, (a_tiles + 2) * 8},
                              {"uctx.cnt", s.kd.uctx.cnt, uctx * 8},
                              {"uctx.node", s.kd.uctx.node, uctx * 4},
                              {"cu_tmp", s.kd.cu_tmp, 0}};
  if (diffs) {
    regs.push_back({"dv_old", s.kd.dv_old, m * 8});
    regs.push_back({"dv_new", s.kd.dv_new, m * 8});
  } else {
    CHECK(!s.kd.dv_old && !s.kd.dv_new, "winners without diffs");
  }
  CHECK(s.ed.cap == e_rows && s.ed.n == 0 && s.kd.uctx.cap == uctx, "capacities");
  CHECK((char*)s.tabC + s.zero_bytes == (char*)s.e_next + 256, "zeroed: %zu bytes from tabC", s.zero_bytes);
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
  const u64 ITEMS[] = {1, 2, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 12800, 100003};
  for (u64 k : {u64(1), u64(2), u64(17), u64(63), u64(64)})
    for (u64 m : ITEMS)
      for (size_t sb : {size_t(0), size_t(257), size_t(100001)})
        for (u64 er : {u64(0), u64(1), u64(31), u64(32), u64(33), u64(12797)})
          for (bool diffs : {false, true}) run(k, m, sb, er, (m * 7) % 19, k + 3, diffs);
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
