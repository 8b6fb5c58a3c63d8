// The scratch layouts of csrc/dg_arena.h, checked on the host (tests/test_arena_layouts.py
// builds this with ASan and UBSan and runs it).  For every layout and shape: the measuring
// and the carving pass agree, every region lies inside the buffer, is aligned for its type
// (8-byte columns of a store for the 16-byte pair moves), overlaps no other, sits at the
// offset the hand-written formulas of the single-file C-ABI layer gave it (restated below
// as plain arithmetic, one table per layout), and its first and last element can be written
// in a block of exactly bytes().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dg_arena.h"

using namespace dg;
typedef uint64_t u64;

static int g_fail = 0;
static long g_checked = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (g_fail++ < 20) {                     \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                   \
        printf("\n");                          \
      }                                        \
    }                                          \
  } while (0)

static size_t al(size_t b) { return (b + 255) / 256 * 256; }

struct Region {
  const char* name;
  const void* p;
  size_t bytes, elem, align, want;  // want: the offset the old formulas give
};

// the five columns of a store at `base`, old carve_store order and rounding
static void store_regions(std::vector<Region>& r, const char* name, const dg_store& s, u64 rows, size_t base) {
  const size_t c = al(rows * 8);
  r.push_back({name, s.key, rows * 8, 8, 16, base});
  r.push_back({name, s.val, rows * 8, 8, 16, base + c});
  r.push_back({name, s.ts, rows * 8, 8, 16, base + 2 * c});
  r.push_back({name, s.cnt, rows * 8, 8, 16, base + 3 * c});
  r.push_back({name, s.node, rows * 4, 4, 8, base + 4 * c});
}
static size_t store_bytes(u64 rows) { return 4 * al(rows * 8) + al(rows * 4); }

// One layout at one shape.  `layout(Arena&, std::vector<Region>&)` carves and lists its
// regions; old_total: the bytes the old formula asked for.
template <class Layout>
static void run(const char* what, size_t old_total, Layout layout) {
  std::vector<Region> none, regs;
  Arena measure;
  layout(measure, none);
  const size_t total = measure.bytes();
  char* blk = (char*)aligned_alloc(256, total);
  Arena real(blk);
  layout(real, regs);
  CHECK(real.off == measure.off, "%s: measured %zu, carved %zu", what, measure.off, real.off);
  CHECK(total % 256 == 0 && total >= measure.off, "%s: total %zu for %zu", what, total, measure.off);
  CHECK(total <= (al(old_total) > 256 ? al(old_total) : 256), "%s: total %zu > old %zu", what, total, old_total);
  for (size_t i = 0; i < regs.size(); i++) {
    const Region& g = regs[i];
    const size_t off = (const char*)g.p - blk;
    CHECK(g.p != nullptr, "%s %s[%zu]: null", what, g.name, i);
    CHECK(off == g.want, "%s %s[%zu]: offset %zu, was %zu", what, g.name, i, off, g.want);
    CHECK(off + g.bytes <= total, "%s %s[%zu]: ends at %zu of %zu", what, g.name, i, off + g.bytes, total);
    CHECK(off % g.align == 0, "%s %s[%zu]: offset %zu not %zu-aligned", what, g.name, i, off, g.align);
    for (size_t j = 0; j < i; j++) {
      const size_t o2 = (const char*)regs[j].p - blk;
      CHECK(!g.bytes || !regs[j].bytes || off + g.bytes <= o2 || o2 + regs[j].bytes <= off,
            "%s: %s[%zu] overlaps %s[%zu]", what, g.name, i, regs[j].name, j);
    }
    if (g.bytes) {  // first and last element (ASan: inside the block)
      memset(blk + off, 0x5a, g.elem);
      memset(blk + off + g.bytes - g.elem, 0xa5, g.elem);
    }
    g_checked++;
  }
  free(blk);
}

static const u64 SIZES[] = {0, 1, 31, 32, 33, 255, 256, 257};

static void test_context() {  // join_delta_core's ubuf
  for (u64 cap : SIZES)
    run("context", (cap * 12 + 1024 + 255) / 256 * 256, [&](Arena& a, std::vector<Region>& r) {
      dg_context c = a.context(cap);
      r.push_back({"cnt", c.cnt, cap * 8, 8, 8, 0});
      r.push_back({"node", c.node, cap * 4, 4, 4, (cap * 8 + 255) / 256 * 256});
    });
}

static void test_join() {
  for (u64 ctx : SIZES)
    for (u64 pass : {u64(0), u64(1), u64(257), u64(4096)})
      for (u64 chg : {u64(0), u64(33), u64(1000)})
        run("join", al(ctx) + al(pass) + chg, [&](Arena& a, std::vector<Region>& r) {
          JoinScratch s = join_layout(a, ctx, pass, chg);
          r.push_back({"ctx", s.ctx, ctx, 1, 256, 0});
          r.push_back({"pass", s.pass, pass, 1, 256, al(ctx)});
          if (chg) r.push_back({"chg", s.chg, chg, 1, 256, al(ctx) + al(pass)});
          else CHECK(s.chg == nullptr, "join: chg without change events");
        });
}

// The three layouts the join's launchers carve (join*.hip) and join2_enqueue measures: the
// old offsets are launch_join2's place_splits and pass carve, join.hip's chg_layout, and the
// byte formulas of dg_launch.h (join2_pass_tmp_bytes, join2_changes_tmp_bytes) and
// api_join.hip (3 * tiles + 3 state words).
static const u64 JOIN_TILES[] = {0, 1, 63, 64, 65, 129, 4096};
static const u64 JT = 1016, JOIN_MAX_GRID = 2048;  // JOIN_TILE; join2_tiles_cap's margin

static void test_join_state() {
  for (u64 t : JOIN_TILES)
    for (u64 n : {t, t + JOIN_MAX_GRID})
      run("join state", (3 * n + 3) * 8, [&](Arena& a, std::vector<Region>& r) {
        JoinState s = join_state_layout(a, n);
        r.push_back({"splits", s.splits, (n + 1) * 8, 8, 8, n * 8});
        r.push_back({"ksplits", s.ksplits, (n + 1) * 8, 8, 8, (2 * n + 1) * 8});
        CHECK(a.off == (3 * n + 2) * 8, "join state: %zu bytes for %llu tiles", a.off, (unsigned long long)n);
      });
}

static void test_pass() {
  for (u64 n : JOIN_TILES)
    run("pass", (n * 4 + 255) / 256 * 256 + n * JT * 2 + 256, [&](Arena& a, std::vector<Region>& r) {
      PassScratch s = pass_layout(a, n, JT);
      r.push_back({"counts", s.counts, n * 4, 4, 4, 0});
      r.push_back({"lists", s.lists, n * JT * 2, 2, 2, (n * 4 + 255) / 256 * 256});
    });
}

static void test_chg() {
  for (u64 n : JOIN_TILES)
    run("chg", n * (JT * 8 + 8 + 12 + 16) + 8 + 256, [&](Arena& a, std::vector<Region>& r) {
      ChgScratch s = chg_layout(a, n, JT);
      const size_t off = n * JT * 8, cnt = off + n * 8, fk = (cnt + 3 * n * 4 + 7) / 8 * 8;
      r.push_back({"ev", s.ev, n * JT * 8, 8, 8, 0});
      r.push_back({"chunk", s.chunk, n * 8, 8, 8, off});
      r.push_back({"cnt", s.cnt, n * 4, 4, 4, cnt});
      r.push_back({"wu", s.wu, n * 4, 4, 4, cnt + n * 4});
      r.push_back({"fk", s.fk, n * 8, 8, 8, fk});
      r.push_back({"lk", s.lk, n * 8, 8, 8, fk + n * 8});
      // the chunk summaries written: one of 32 bytes per 64 tiles, but the last
      const u64 written = n ? (n + 63) / 64 - 1 : 0;
      CHECK(CHG_CHUNK == 64 && CHG_SUM_BYTES == 32, "chg: chunk constants");
      const size_t room = a.base ? (size_t)((const char*)s.cnt - (const char*)s.chunk) : n * 8;
      CHECK(written * 32 <= room, "chg: %llu summaries in %zu bytes", (unsigned long long)written, room);
    });
}

static void test_splice() {
  for (u64 rows : SIZES)
    for (u64 nk : SIZES)
      for (u64 uc : {u64(0), u64(33)}) {
        const u64 cap_k = rows, cap_e = rows + nk, tiles = rows / 32;
        const size_t idx = ((nk + 1) * 8 + 255) / 256 * 256, tile_bytes = ((tiles + 1) * 8 + 255) / 256 * 256;
        const size_t ctx_bytes = (uc * 12 + 2 * 256) / 256 * 256 + 256;
        const size_t old = ((cap_k * 36 + 5 * 256) + (cap_e * 36 + 5 * 256) + 5 * idx + tile_bytes + ctx_bytes + 256 + 255) /
                           256 * 256;
        run("splice", old, [&](Arena& a, std::vector<Region>& r) {
          SpliceScratch s = splice_layout(a, cap_k, cap_e, nk, tiles, uc);
          store_regions(r, "ak", s.ak, cap_k, 0);
          store_regions(r, "ed", s.ed, cap_e, store_bytes(cap_k));
          const size_t p = store_bytes(cap_k) + store_bytes(cap_e);
          r.push_back({"a_lo", s.idx.a_lo, (nk + 1) * 8, 8, 8, p});
          r.push_back({"a_off", s.idx.a_off, (nk + 1) * 8, 8, 8, p + idx});
          r.push_back({"end", s.idx.end, (nk + 1) * 8, 8, 8, p + 2 * idx});
          r.push_back({"shift", s.idx.shift, (nk + 1) * 8, 8, 8, p + 3 * idx});
          r.push_back({"gap", s.idx.gap, (nk + 1) * 8, 8, 8, p + 4 * idx});
          r.push_back({"tile_u0", s.tile_u0, (tiles + 1) * 8, 8, 8, p + 5 * idx});
          r.push_back({"uctx.cnt", s.uctx.cnt, uc * 8, 8, 8, p + 5 * idx + tile_bytes});
          r.push_back({"uctx.node", s.uctx.node, uc * 4, 4, 4, p + 5 * idx + tile_bytes + (uc * 8 + 255) / 256 * 256});
          CHECK(s.ak.cap == cap_k && s.ed.cap == cap_e && s.uctx.cap == uc && s.ak.n == 0, "splice: caps");
        });
      }
}

static void test_kd() {
  for (u64 nk : SIZES)
    for (u64 rows : SIZES)
      for (int diffs = 0; diffs < 2; diffs++) {
        const u64 ntiles = (nk + 255) / 256, part = ntiles * 7, a_tiles = rows / 16, uc = rows % 40, cu_bytes = 24 * uc + 8;
        const size_t per_key = al(nk * 8), per_key1 = al((nk + 1) * 8), tiles_b = al(part * 8);
        const size_t tu = al((a_tiles + 2) * 8), uc_b = al(uc * 8) + al(uc * 4), cu_b = al(cu_bytes);
        const size_t old = (diffs ? 9 : 7) * per_key + per_key1 + tiles_b + tu + uc_b + cu_b;
        run("kd", old, [&](Arena& a, std::vector<Region>& r) {
          KdScratch s = kd_layout(a, nk, part, a_tiles, uc, cu_bytes, diffs != 0);
          const void* keyed[7] = {s.a_lo, s.d_lo, s.runs, s.amask, s.dmask, s.dh, s.end};
          for (int i = 0; i < 7; i++) r.push_back({"per-key", keyed[i], nk * 8, 8, 8, i * per_key});
          size_t p = 7 * per_key;
          r.push_back({"shift", s.shift, (nk + 1) * 8, 8, 8, p});
          r.push_back({"part", s.part, part * 8, 8, 8, p += per_key1});
          r.push_back({"tile_u0", s.tile_u0, (a_tiles + 2) * 8, 8, 8, p += tiles_b});
          r.push_back({"uc_cnt", s.uctx.cnt, uc * 8, 8, 8, p += tu});
          r.push_back({"uc_node", s.uctx.node, uc * 4, 4, 4, p += al(uc * 8)});
          r.push_back({"cu_tmp", s.cu_tmp, cu_bytes, 1, 256, p += al(uc * 4)});
          if (diffs) {
            r.push_back({"dv_old", s.dv_old, nk * 8, 8, 8, p += cu_b});
            r.push_back({"dv_new", s.dv_new, nk * 8, 8, 8, p += per_key});
          } else {
            CHECK(!s.dv_old && !s.dv_new, "kd: winners without diffs");
          }
        });
      }
}

static void test_home() {
  const u64 EDIT = 1536, WORDS = 8 + 512 + 4 * 1536 + 1536 / 2 + 2048 + 2048 / 2;  // SMALL_EDIT, SMALL_WORDS
  for (u64 nk : SIZES)
    for (u64 a_tiles : SIZES) {
      const size_t idx = ((nk + 1) * 8 + 255) / 256 * 256;
      const size_t old = (EDIT * 36 + 5 * 256) + 6 * idx + ((a_tiles + 2) * 8 + 255) / 256 * 256 + 256 + WORDS * 8 + 256;
      run("home", old, [&](Arena& a, std::vector<Region>& r) {
        HomeScratch s = home_layout(a, EDIT, nk, a_tiles, WORDS);
        store_regions(r, "ed", s.ed, EDIT, 0);
        size_t q = store_bytes(EDIT);
        r.push_back({"a_lo", s.idx.a_lo, (nk + 1) * 8, 8, 8, q});
        r.push_back({"a_off", s.idx.a_off, (nk + 1) * 8, 8, 8, q + idx});
        r.push_back({"end", s.idx.end, (nk + 1) * 8, 8, 8, q + 2 * idx});
        r.push_back({"shift", s.idx.shift, (nk + 1) * 8, 8, 8, q + 3 * idx});
        r.push_back({"gap", s.idx.gap, (nk + 1) * 8, 8, 8, q + 4 * idx});
        q += 6 * idx;
        r.push_back({"tile_u0", s.tile_u0, (a_tiles + 2) * 8, 8, 8, q});
        q += ((a_tiles + 2) * 8 + 255) / 256 * 256;
        r.push_back({"moved", s.moved, 4, 4, 8, q});
        r.push_back({"res", s.res, WORDS * 8, 8, 8, q + 256});
      });
    }
}

static void test_tree() {
  for (u64 chunks : {u64(1), u64(2), u64(3), u64(31), u64(32), u64(33), u64(255), u64(256), u64(257)}) {
    const u64 cw = 4 * chunks, cpad = (chunks + 1) & ~1ull, zw = cpad + 2 * chunks;
    // dg_merkle_update: everything in one buffer
    run("tree", (cw + zw) * 4, [&](Arena& a, std::vector<Region>& r) {
      TreeScratch s = tree_layout(a, a, cw, chunks);
      r.push_back({"hand", s.hand, cw * 4, 8, 8, 0});
      r.push_back({"dirty", s.dirty, cpad * 4, 4, 4, cw * 4});
      r.push_back({"cdelta", s.cdelta, chunks * 8, 8, 8, (cw + cpad) * 4});
      CHECK(s.zero_words == zw, "tree: zero_words %llu, was %llu", (unsigned long long)s.zero_words, (unsigned long long)zw);
    });
    // the one-wait path: the flags and changes in their own buffer (checked as the layout's
    // second arena; the first one only measures here)
    run("tree flags", zw * 4, [&](Arena& a, std::vector<Region>& r) {
      Arena hand;
      TreeScratch s = tree_layout(hand, a, cw, chunks);
      CHECK(hand.off == cw * 4 && s.hand == nullptr, "tree: hand words %zu", hand.off);
      r.push_back({"dirty", s.dirty, cpad * 4, 4, 4, 0});
      r.push_back({"cdelta", s.cdelta, chunks * 8, 8, 8, cpad * 4});
    });
  }
}

static void test_fold() {  // packed: odd and even totals
  for (u64 rows : SIZES)
    for (u64 ctx : {u64(0), u64(1), u64(2), u64(33)}) {
      const size_t half = ((rows * 36 + ctx * 12 + 1024) + 255) / 256 * 256;
      run("fold", 2 * half, [&](Arena& a, std::vector<Region>& r) {
        FoldScratch s = fold_layout(a, rows, ctx);
        for (int w = 0; w < 2; w++) {
          size_t p = w * half;
          r.push_back({"key", s.st[w].key, rows * 8, 8, 8, p});
          r.push_back({"val", s.st[w].val, rows * 8, 8, 8, p += rows * 8});
          r.push_back({"ts", s.st[w].ts, rows * 8, 8, 8, p += rows * 8});
          r.push_back({"cnt", s.st[w].cnt, rows * 8, 8, 8, p += rows * 8});
          r.push_back({"cx.cnt", s.cx[w].cnt, ctx * 8, 8, 8, p += rows * 8});
          r.push_back({"node", s.st[w].node, rows * 4, 4, 4, p += ctx * 8});
          r.push_back({"cx.node", s.cx[w].node, ctx * 4, 4, 4, p += rows * 4});
          CHECK(s.st[w].cap == rows && s.cx[w].cap == ctx && s.st[w].n == 0 && s.cx[w].n == 0 &&
                    s.cx[w].kind == DG_CTX_VV,
                "fold: caps");
          // what decides whether an intermediate splices: 16-byte columns iff rows is even
          const bool pair = !(((uintptr_t)s.st[w].key | (uintptr_t)s.st[w].val | (uintptr_t)s.st[w].ts |
                               (uintptr_t)s.st[w].cnt) & 15) && !((uintptr_t)s.st[w].node & 7);
          CHECK(!a.base || pair == (rows % 2 == 0), "fold: rows %llu pair-aligned %d", (unsigned long long)rows, (int)pair);
        }
      });
    }
}

static void test_kfold() {
  const u64 RUN = 72, KNT = 1024;  // a run descriptor's bytes (any size: a parameter), the VV tables' nodes
  for (u64 k : {u64(1), u64(2), u64(64)})
    for (u64 T : {u64(1), u64(31), u64(32), u64(33), u64(257)})
      for (u64 dset_n : {u64(0), u64(1024), u64(4096)}) {  // without and with a DOTS delta
        const size_t b_runs = al(k * RUN), b_cf = al((k + 1) * 8), b_ss = al((T + 1) * 8);
        const size_t b_ds = al((T + 1) * 2 * k * 4), b_tab = al(k * KNT * 8), b_dset = dset_n ? al(dset_n * 8) : 0;
        run("kfold", b_runs + b_cf + b_ss + b_ds + 2 * b_tab + 256 + b_dset, [&](Arena& a, std::vector<Region>& r) {
          KfoldScratch s = kfold_layout(a, k, RUN, T, KNT, dset_n);
          r.push_back({"runs", s.staged.runs, k * RUN, 1, 256, 0});
          r.push_back({"cflat", s.staged.cflat, (k + 1) * 8, 8, 8, b_runs});
          size_t p = b_runs + b_cf;
          CHECK(s.staged_bytes == p, "kfold: staged %zu, was %zu", s.staged_bytes, p);
          r.push_back({"sstart", s.sstart, (T + 1) * 8, 8, 8, p});
          r.push_back({"dstart", s.dstart, (T + 1) * 2 * k * 4, 4, 4, p += b_ss});
          r.push_back({"tabC", s.tabC, k * KNT * 8, 8, 8, p += b_ds});
          r.push_back({"tabP", s.tabP, k * KNT * 8, 8, 8, p += b_tab});
          r.push_back({"flag", s.flag, 4, 4, 4, p += b_tab});
          CHECK(s.zero_bytes == b_ss + b_ds + 2 * b_tab + 256, "kfold: zeroed %zu", s.zero_bytes);
          if (dset_n) r.push_back({"dset", s.dset, dset_n * 8, 8, 8, p + 256});
          else CHECK(s.dset == nullptr, "kfold: a dot set without dots");
          // the pinned staging carves the same head
          Arena st(a.base);
          KfoldStaged h = kfold_staged_layout(st, k, RUN);
          CHECK(h.runs == s.staged.runs && h.cflat == s.staged.cflat && st.off == s.staged_bytes, "kfold: staging");
        });
      }
}

static void test_mutate() {
  for (u64 n : SIZES)
    for (u64 sort_b : {u64(0), u64(256), u64(2048)}) {
      const size_t n4 = al(n * 4), n8 = al(n * 8);
      run("mutate", 2 * (n4 + n8) + sort_b + 256, [&](Arena& a, std::vector<Region>& r) {
        MutateScratch s = mutate_layout(a, n, sort_b);
        r.push_back({"dnode", s.dnode, n * 4, 4, 4, 0});
        r.push_back({"dcnt", s.dcnt, n * 8, 8, 8, n4});
        r.push_back({"tnode", s.tnode, n * 4, 4, 4, n4 + n8});
        r.push_back({"tcnt", s.tcnt, n * 8, 8, 8, 2 * n4 + n8});
        r.push_back({"sort", s.sort_tmp, sort_b, 1, 256, 2 * (n4 + n8)});
      });
    }
}

static void test_mark() {
  const u64 SEG = 24, LDS_IDS = 2048;  // a column descriptor's bytes (a parameter), MARK_LDS_IDS
  for (u64 n_stores : SIZES)
    for (u64 words : SIZES) {
      const size_t seg_bytes = ((n_stores + 1) * SEG + 255) / 256 * 256, bm = (words * 4 + 255) / 256 * 256;
      run("mark", seg_bytes + bm + LDS_IDS * 8, [&](Arena& a, std::vector<Region>& r) {
        MarkScratch s = mark_layout(a, n_stores, SEG, words, LDS_IDS);
        r.push_back({"segs", s.segs, (n_stores + 1) * SEG, 1, 8, 0});
        r.push_back({"bitmap", s.bitmap, words * 4, 4, 4, seg_bytes});
        r.push_back({"samples", s.samples, LDS_IDS * 8, 8, 8, seg_bytes + bm});
      });
    }
}

int main() {
  test_context();
  test_join();
  test_join_state();
  test_pass();
  test_chg();
  test_splice();
  test_kd();
  test_home();
  test_tree();
  test_fold();
  test_kfold();
  test_mutate();
  test_mark();
  printf("%ld regions checked, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
