// join.hip — AWLWWMap.join/3 on gfx950 (reference lib/delta_crdt/aw_lww_map.ex:153-209):
// launch_join2, which chooses the kernels of a join, and the two kernels beside the tiles.
// (The formulation, and what one tile does: dg_jtile.h.)
//
// Kernel shape (HBM-bound integer merge; no MFMA):
//   1. join2_partition_kernel: one wave per tile boundary finds the merge-path split
//      of diagonal q*jt (jt = JT, or less: balance_tiles; the search: dg_jsplit.h).  One
//      extra workgroup (the grid's first) computes the context union Dots.union(c1, c2)
//      (:155).
//   2. join2_stream_kernel (join_stream.hip; single pass, the default): a persistent grid
//      of resident workgroups merges the tiles and writes the kept rows.  A join of at
//      most FUSE_IT tiles per workgroup is ONE launch: the stream kernel searches its own
//      splits and one more workgroup computes the context union (no step 1).
//   (join2_slot_kernel + join2_compact_kernel, join_twopass.hip: the two-pass variant
//    behind step 1, the fallback when a stream grid aborted, and selected with
//    DG_JOIN_MODE=2 for A/B measurement.)
// The changed keys of a join (dg_join2_changes): join_changes.hip, from the events the
// stream kernel records.
#include <algorithm>

#include "dg_arena.h"
#include "dg_jsplit.h"
#include "dg_jtile.h"

namespace dg {

namespace {

// ------------------------------------------------------------- context union
// (Dots.union/2, aw_lww_map.ex:39-52: dg_ctxu.h; here its standalone one-workgroup kernel)
constexpr int CB = 1024;  // threads of the standalone context-union kernel

__global__ __launch_bounds__(CB) void ctx_union_kernel(CtxUnionArgs p) {
  __shared__ u32 s_wave[CB / WAVE + 1];
  ctx_union_block<CB>(p, s_wave);
}

__global__ __launch_bounds__(PB) void join2_partition_kernel(Rows A, Rows B, u64 ntiles, u64 jt,
                                                             u64* splits, CtxUnionArgs cu,
                                                             const u64* keys, u64 n_keys,
                                                             u64* ksplits) {
  // the extra workgroup computes Dots.union(c1, c2) (aw_lww_map.ex:155); it is the FIRST
  // of the grid so its latency chain runs beside the searches instead of after the last
  // of them has been dispatched (config 5: partition 20.4 -> 18.1 us, A/B)
  if (blockIdx.x == 0) {
    __shared__ u32 s_wave[PB / WAVE + 1];
    ctx_union_block<PB>(cu, s_wave);
    return;
  }
  const u64 q = (u64)(blockIdx.x - 1) * (PB / WAVE) + (threadIdx.x >> 6);
  if (q > ntiles) return;
  const u64 d = min(q * jt, A.n + B.n);
  const u64 s = mp_split(A, B, d);
  if ((threadIdx.x & (WAVE - 1)) == 0) splits[q] = s;
  if (keys) {
    const u64 kq = key_split(A, B, keys, n_keys, d, s);
    if ((threadIdx.x & (WAVE - 1)) == 0) ksplits[q] = kq;
  }
}

}  // namespace

// A stream grid of G workgroups runs ceil(ntiles / G) stripes, the last one partly
// idle (config 2: 1969 tiles of 1016 positions on 512 workgroups, the fourth stripe 433
// tiles).  The tiles are re-cut to jt = ceil(total / (stripes x G)) <= JT positions, so
// every stripe is full and each of them carries less: ntiles grows by less than G
// (join2_tiles_cap sizes the scratch).  Fused joins only (at most FUSE_IT stripes, so a
// part-idle last stripe is a large share): config 2 34.3-35.0 against 36.4-38.6 us per
// join (A/B, one box).  The long partitioned joins keep JT (config 5 measured 368-370
// against 340-344 us re-cut, one stripe in 44 being part idle), and so do the
// changed-keys joins, whose event scratch is laid out by join2_tiles.
static void balance_tiles(JoinArgs& p, u64 G) {
  const u64 total = p.a.n + p.b.n;
  if (G == 0 || p.ntiles <= G) return;
  const u64 k = (p.ntiles + G - 1) / G;
  // (even, as JT is: two replicas of the same keys merge in pairs, so an even diagonal is
  // split exactly by the proportional guess the fused kernel checks first -- odd tiles
  // sent half the boundaries to the search: 42.4 against 35.1 us at config 2)
  const u64 jt = std::min<u64>(((total + k * G - 1) / (k * G) + 1) & ~1ull, JT);
  p.jt = jt;
  p.ntiles = (total + jt - 1) / jt;
}

hipError_t launch_join2(const Rows& a, const Ctx& ca, const Rows& b, const Ctx& cb,
                        const u64* keys, u64 n_keys, const RowsOut& out, u32* out_ctx_node,
                        u64* out_ctx_cnt, void* ctx_tmp, void* pass_tmp, int mode,
                        const Scan& scan, int workers, u64* d_counts, hipStream_t st,
                        void* chg_tmp, int stagger) {
  JoinArgs p;
  p.a = a;
  p.b = b;
  p.ca = ca;
  p.cb = cb;
  p.keys = keys;
  p.n_keys = n_keys;
  p.ntiles = join2_tiles(a.n, b.n);
  p.jt = JT;
  // the splits and the keyset splits (keyed joins) in scan.state; placed again when the
  // tiles are re-cut (balance below)
  JoinState js;
  auto place_splits = [&]() {
    Arena state(scan.state);
    js = join_state_layout(state, p.ntiles);
    p.splits = js.splits;
    p.ksplits = js.ksplits;
  };
  place_splits();
  const CtxUnionArgs cu = make_cu(ca, cb, out_ctx_node, out_ctx_cnt, d_counts + 1, ctx_tmp);
  p.out = out;
  p.scan = scan;
  p.d_count = d_counts;
  p.lists = nullptr;
  p.counts = nullptr;
  p.chg_tmp = nullptr;
  p.chg_cnt = p.chg_wu = nullptr;
  p.chg_fk = p.chg_lk = nullptr;
  if (chg_tmp) {
    Arena arena(chg_tmp);
    const ChgScratch l = chg_layout(arena, p.ntiles, JT);
    p.chg_tmp = l.ev;
    p.chg_cnt = l.cnt;
    p.chg_wu = l.wu;
    p.chg_fk = l.fk;
    p.chg_lk = l.lk;
  }
  if (p.ntiles == 0) {
    // no rows: only the context union runs.  (No tile kernel below is launched without
    // rows: slot_row clamps a load's index into a store that has some.)
    hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(u64), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ctx_union_kernel, dim3(1), dim3(CB), 0, st, cu);
    return hipGetLastError();
  }
  // two version vectors: LDS VV tables; a key list: per-tile keyset slices
  const bool fast = ca.kind == 0 && cb.kind == 0;
  const bool keyed = keys != nullptr;
  p.stagger = stagger;
  p.cu = cu;
  const StreamKernels sk = stream_kernels(fast, keyed, chg_tmp != nullptr);
  auto kern = sk.part;
  auto kern_late = sk.fused;  // the fused launch
  const bool stream = mode != JOIN_TWO_PASS || chg_tmp;
  u64 g = 0;
  if (stream) {
    g = workers > 0 ? (u64)workers : resident_grid((const void*)kern);
    g = std::min<u64>(std::min<u64>(p.ntiles, g), (u64)CQ * JB);  // stripe counts: CQ per thread
    // small joins (<= FUSE_IT tiles per workgroup): the splits are searched inside the
    // stream kernel and the context union runs in one extra co-resident workgroup, so
    // the partition launch (~5 us of mostly fixed cost) disappears
    static const bool no_fuse = [] {
      const char* v = getenv("DG_JOIN_FUSE");
      return v && v[0] == '0';
    }();
    const u64 gr = workers > 0 ? g + 1 : resident_grid((const void*)kern_late);
    const u64 gt = std::min<u64>(std::min<u64>(p.ntiles, gr - 1), (u64)CQ * JB);
    if (!no_fuse && gr >= 2 && p.ntiles <= (u64)FUSE_IT * gt) {
      if (!chg_tmp) balance_tiles(p, gt);
      place_splits();
      return launch_stream(kern_late, gt + 1, p, st);
    }
  }
  const u64 nb_part = (p.ntiles + 1 + (PB / WAVE) - 1) / (PB / WAVE);
  hipLaunchKernelGGL(join2_partition_kernel, dim3((unsigned)nb_part + 1), dim3(PB), 0, st, a, b,
                     p.ntiles, p.jt, js.splits, cu, keys, n_keys, js.ksplits);
  if (!stream) return launch_two_pass(p, fast, keyed, pass_tmp, st);
  return launch_stream(kern, g, p, st);
}

hipError_t launch_ctx_union(const Ctx& a, const Ctx& b, u32* out_node, u64* out_cnt,
                            u64* d_count, void* tmp, hipStream_t st) {
  CtxUnionArgs p = make_cu(a, b, out_node, out_cnt, d_count, tmp);
  hipLaunchKernelGGL(ctx_union_kernel, dim3(1), dim3(CB), 0, st, p);
  return hipGetLastError();
}

}  // namespace dg
