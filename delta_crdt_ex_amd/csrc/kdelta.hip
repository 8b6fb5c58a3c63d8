// kdelta.hip — update_state_with_delta for a keyed delta of ANY size with one host wait.
//
// CausalCrdt joins every sync delta and every batch of local mutations into the replica
// with its keyset (reference causal_crdt.ex:383-394; aw_lww_map.ex:153-209).  When the
// delta's keys all lie in the keyset, only the keyset's keys change, and each key's new
// rows are join_dot_sets/4 (:196-209) of its state rows and its delta rows -- a handful of
// rows per key.  So instead of a merge-path join of the taken rows (whose launch is sized
// by counts the host must wait for), every keyset key is one thread:
//
//   kd_count_kernel   (one thread per key) its state run (an interpolation search of the
//                     state: key ids are hashes) and delta run, the per-key join: which
//                     state rows stay (s1 ∩ s2 ∪ s1 \ c2) and which delta rows come in
//                     (s2 \ c1) -- kept as two bit masks -- whether the key changed (diff/3,
//                     causal_crdt.ex:344-352) and its Merkle leaf change (Σ row_hash new -
//                     Σ row_hash old), put into the tree right away (segmented wave sums:
//                     one atomic per bucket and chunk); per workgroup the sums of rows, kept
//                     rows, changed keys and their rows, delta rows seen; the last key
//                     workgroup to finish sums them into the totals and the guard word: a
//                     delta row outside the keyset (the right-biased carry of :185-188
//                     applies: the caller runs the full join), a key run over KD_RUN rows,
//                     more changed keys than the caller's capacity.  Workgroup 0 of the
//                     launch computes the context union (Dots.union/2).
//                     kd_count_diffs_kernel (dg_join_delta_diffs) is the same walk that also
//                     keeps read/1's winner of the key's rows before and after the join.
//   kd_finish_kernel  (merkle_build.hip + dg_kdw.h, one launch) one thread per key: its new rows --
//                     in place when no key's row count changed (and no key's in-place
//                     write would read back a row it wrote: KD_MOVED), else straight to their
//                     final places in the spare store -- the changed keys and their rows
//                     (device or page-locked host memory), the splice index of the rows
//                     that move (splice.hip), the union context into the state's; every
//                     state write skipped when the tree update reported an input error (all
//                     or nothing); each workgroup sums the earlier count workgroups'
//                     figures for its offsets.  Beside them, persistent workgroups re-reduce
//                     the dirty chunks of the tree (update_hashes).
//   splice_kernel     (splice.hip, only when rows moved) the untouched rows to the spare
//
// then the count block is published to mapped host memory and the host waits ONCE.
//
// dg_join_deltas_keyed (the fold of k small keyed deltas) runs the same chain with
// kk_count_kernel in kd_count_kernel's place: a thread per key of the keysets' union
// evaluates kfold.hip's rule and leaves the key's new rows in an edit store that the write
// reads as its delta (kkeyed.hip).  dg_kdcount.h holds what the two count kernels share: the
// tree's put/delete and the tail that writes the count block.
//
// Roofline: each key costs two searches (~6 dependent loads of the state, a few of the
// delta) and reads its few rows twice (the second time from L2); a sync delta of 125k keys
// into a 12.5M-row state reads ~10 MB.  Latency-bound by the search chains, not by bytes.
#include "dg_ctxu.h"
#include "dg_hash.h"
#include "dg_launch.h"

#ifdef DG_STAMPS
// Diagnostic build only (DG_STAMPS=1): per-workgroup timestamps (s_memrealtime, 100 MHz) of
// the count kernel, read back with dg_debug_kd_stamps (tools/kd_stamps.py).  No barriers
// added: thread `th` stamps slot k when it passes that point.  (Ahead of dg_kdcount.h: the
// last two stamps are in kd_count_tail.)
namespace dg {
namespace {
__device__ u64 g_kd_stamps[4096 * 8];
#define KDSTAMP(th, k)                                                        \
  do {                                                                        \
    if (threadIdx.x == (th) && blk < 4096)                                    \
      g_kd_stamps[blk * 8 + (k)] = __builtin_amdgcn_s_memrealtime();          \
  } while (0)
}  // namespace
}  // namespace dg
#endif
#include "dg_kdcount.h"

namespace dg {

namespace {

constexpr u32 KVT = 1024;  // VV tables in LDS cover node ids < KVT

// Map.get(vv, node, 0) >= cnt through the LDS table (node ids < KVT), else a search
__device__ __forceinline__ bool vv_covers(const u64* tab, const Ctx& c, u32 n, u64 cnt) {
  if (n < KVT) return tab[n] >= cnt;
  return ctx_covers(c.node, c.cnt, c.n, 0, n, cnt);
}

// ---------------------------------------------------------------- count (+ scan)
// The workgroup's keys are ascending, so their delta rows are one contiguous range: two
// searches find its ends and its keys are staged in LDS (every key's delta run is found
// there, not by a search of the delta in memory).  (Narrowing the state searches to the
// workgroup's range the same way, by 64-ary wave searches, measured slower: 52 against
// 45 us at config 4 -- their 256 scattered lines per bound outweigh what each key saves.)
constexpr u32 KDL = 2048;  // delta keys staged per workgroup (more: searched in memory)
// DIFFS: the walk also keeps read/1's winner (aw_lww_map.ex:211-224) of the key's rows before
// and after the join -- a key's rows come in (val, ts) order on both sides and the merge
// visits them in that order, so "a row wins only on a strictly greater ts" (segred.hip) is
// one compare per row here -- for dg_join_delta_diffs (causal_crdt.ex:361-381).  Compiled
// out of kd_count_kernel: the other entry points run the code they ran before.
template <bool DIFFS>
__device__ __forceinline__ void kd_count_body(const KdArgs& p) {
  __shared__ u64 tabS[KVT], tabD[KVT];
  __shared__ u64 s_dk[KDL];
  __shared__ u64 s_rng[2];
  __shared__ u32 s_cw[KDB / WAVE + 1];
  if (blockIdx.x == 0) {
    // Dots.union(state context, delta context) (:155) into the union scratch and
    // d_counts[KC_CTX], by a workgroup of its own beside the keys' (it needs only the inputs;
    // in the last workgroup's tail it added ~5 us to every call)
    ctx_union_block<KDB>(make_cu(p.ca, p.cd, p.uc_node, p.uc_cnt, p.d_counts + KC_CTX, p.cu_tmp), s_cw);
    return;
  }
  const u64 blk = blockIdx.x - 1;  // the keys' workgroups: 1 .. ntiles
  const int tid = threadIdx.x;
  const u64 u = blk * KDB + tid;
  const u64 u0 = blk * KDB, u1 = min<u64>(u0 + KDB, p.nk);
  const bool dvv = p.cd.kind == 0;
  KDSTAMP(2, 0);
  if (tid < 2) {  // the workgroup's delta range [lo, hi): its keys' rows (two searches)
    const u64 x = tid ? p.keys[u1 - 1] + 1 : p.keys[u0];  // (key + 1: past the last key's run)
    s_rng[tid] = tid && x == 0 ? p.d.n : interp_lower_bound(p.d.key, 0, p.d.n, x);  // (2^64 - 1)
  }
  KDSTAMP(0, 1);
  for (u32 x = tid; x < KVT; x += KDB) {
    tabS[x] = 0;
    tabD[x] = 0;
  }
  __syncthreads();
  for (u64 i = tid; i < p.ca.n; i += KDB)
    if (p.ca.node[i] < KVT) tabS[p.ca.node[i]] = p.ca.cnt[i];
  if (dvv)
    for (u64 i = tid; i < p.cd.n; i += KDB)
      if (p.cd.node[i] < KVT) tabD[p.cd.node[i]] = p.cd.cnt[i];
  const u64 dlo = s_rng[0], dhi = s_rng[1];
  const bool dl = dhi - dlo <= KDL;  // (uniform)
  if (dl)
    for (u64 i = tid; i < dhi - dlo; i += KDB) s_dk[i] = p.d.key[dlo + i];
  u64 v[KD_NV] = {0, 0, 0, 0, 0, 0, 0};
  u64 a_lo = 0, d_lo = 0, am = 0, dm = 0, dh = 0;
  u32 na = 0, nd = 0, ne = 0;
  bool chg = false, big = false, back = false;
  u32 wo = 0;  // rows the write (dg_kdw.h) has stored when it loads the next kept state row
  u64 k = 0;
  u64 ov = 0, nv = 0;    // (DIFFS) the old and the new winner's value id (no row: 0) ...
  i64 ots = 0, nts = 0;  // ... and ts
  if (u < p.nk) {
    k = p.keys[u];
    key_run<KD_RUN>(p.a.key, p.a.n, k, a_lo, na);  // the state: an interpolation search
  }
  KDSTAMP(2, 2);
  __syncthreads();  // (the tables, the staged delta keys)
  KDSTAMP(2, 3);
  if (u < p.nk) {
    if (dl) {  // the delta run from LDS
      u32 lo = 0, hi = (u32)(dhi - dlo);
      while (lo < hi) {
        const u32 m = (lo + hi) >> 1;
        if (s_dk[m] < k)
          lo = m + 1;
        else
          hi = m;
      }
      u32 e = lo;
      while (e < (u32)(dhi - dlo) && s_dk[e] == k && e - lo <= KD_RUN) e++;
      d_lo = dlo + lo;
      nd = e - lo;
    } else {
      key_run<KD_RUN>(p.d.key, p.d.n, k, d_lo, nd);
    }
    big = na > KD_RUN || nd > KD_RUN;
  }
  if (u < p.nk && !big) {
    // join_dot_sets over the key's rows, both sides in tuple order
    u32 i = 0, j = 0;
    Row ra{}, rb{};
    if (na) ra = load_row(p.a, a_lo);
    if (nd) rb = load_row(p.d, d_lo);
    while (i < na || j < nd) {
      int c;  // -1: the state row first, 1: the delta row first, 0: the same row
      if (i >= na) {
        c = 1;
      } else if (j >= nd) {
        c = -1;
      } else {
        bool lt, eq;
        row_cmp_bf(ra, rb, lt, eq);
        c = eq ? 0 : (lt ? -1 : 1);
      }
      if (c <= 0) {
        // the state's row: kept if the delta has it too, or the delta's context does not
        // cover its dot (Dots.member?, :67-73)
        const bool keep = c == 0 || !(dvv ? vv_covers(tabD, p.cd, ra.node, ra.cnt)
                                          : ctx_covers(p.cd.node, p.cd.cnt, p.cd.n, 1, ra.node, ra.cnt));
        if (DIFFS) {  // (selects, not branches: i == 0 / ne == 0 is "no row so far")
          const bool wo = (i == 0) | (ra.ts > ots);
          ots = wo ? ra.ts : ots;
          ov = wo ? ra.val : ov;
          const bool wn = keep & ((ne == 0) | (ra.ts > nts));
          nts = wn ? ra.ts : nts;
          nv = wn ? ra.val : nv;
        }
        if (keep) {
          back |= wo > i;  // written in place, slot i would hold an output row by then
          am |= 1ull << i;
          ne++;
          wo = ne;
        } else {
          chg = true;
          if (p.has_tree) dh -= rh_row(p.t.th, ra);
        }
        if (c == 0 && ++j < nd) rb = load_row(p.d, d_lo + j);
        if (++i < na) ra = load_row(p.a, a_lo + i);
      } else {
        // the delta's row only: kept unless the state's context covers it
        if (!vv_covers(tabS, p.ca, rb.node, rb.cnt)) {
          if (DIFFS) {
            const bool wn = (ne == 0) | (rb.ts > nts);
            nts = wn ? rb.ts : nts;
            nv = wn ? rb.val : nv;
          }
          dm |= 1ull << j;
          ne++;
          chg = true;
          if (p.has_tree) dh += rh_row(p.t.th, rb);
        }
        if (++j < nd) rb = load_row(p.d, d_lo + j);
      }
    }
    p.a_lo[u] = a_lo;
    p.d_lo[u] = d_lo;
    p.amask[u] = am;
    p.dmask[u] = dm;
    if (DIFFS) {  // (the write puts them beside the changed keys, dg_kdw.h)
      p.dv_old[u] = ov;
      p.dv_new[u] = nv;
    }
  }
  KDSTAMP(2, 4);
  if (u < p.nk) {  // (a key over KD_RUN: no change recorded, so the undo skips it too)
    p.runs[u] = big ? 0ull : kd_run_pack(na, nd, ne, chg);
    p.dh[u] = big ? 0ull : dh;
  }
  // the tree's put/delete right away (all or nothing: a guard or an input error found
  // later makes the host undo it, merkle_build.hip kd_tree_kernel with the opposite sign)
  // (a key over KD_RUN keeps its bucket and chunk as its segment, with nothing to add, as in
  // the undo: were its lane left out, the keys of one bucket or chunk on either side of it
  // would be two runs of lanes, and the second run's sum takes the first's in again)
  if (p.has_tree) tree_put(p, u < p.nk, k, chg && !big, dh, (int)ne - (int)na);
  KDSTAMP(2, 5);
  v[0] = na;
  v[1] = ne;
  v[2] = chg ? 1 : 0;
  v[3] = chg ? ne : 0;
  v[4] = nd;
  v[5] = (u64)(i64)((int)(ne > 0) - (int)(na > 0));
  // rows move (the write goes through the spare store, not in place) when the key's row count
  // changes, and also when the in-place write would read back a row it has just written:
  // dg_kdw.h stores output row o at slot o, and loads kept state row i right after it has
  // stored the kept row before it -- by then it has stored `wo` rows, every kept row and every
  // new row up to there, and wo > i means slot i is gone ([X, Y, Z] -> [D, X, Y] came out
  // [D, X, X]).  A new row behind the kept rows, or before the only kept row, is no hazard
  // and stays in place.  (kkeyed.hip's kk_count_body flags every key of several rows that
  // loses one and gains one: wider, and as safe.)
  const bool moved = ne != na || back;
  v[6] = (big ? KD_BIG : 0u) | (moved ? KD_MOVED : 0u);
  // (the keys' delta runs fall short of the delta: a delta row whose key is outside the keyset)
  kd_count_tail(p, blk, v, [&](u64 n_d) { return n_d != p.d.n; });
}

__global__ __launch_bounds__(KDB) void kd_count_kernel(KdArgs p) { kd_count_body<false>(p); }
__global__ __launch_bounds__(KDB) void kd_count_diffs_kernel(KdArgs p) { kd_count_body<true>(p); }

}  // namespace

#ifdef DG_STAMPS
extern "C" int dg_debug_kd_stamps(unsigned long long* host, size_t n) {
  if (n > 4096 * 8) n = 4096 * 8;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_kd_stamps), n * 8) == hipSuccess ? 0 : -3;
}
#endif

hipError_t launch_kd_join(const KdArgs& p0, hipStream_t st) {
  KdArgs p = p0;
  p.ntiles = (p.nk + KDB - 1) / KDB;
  if (p.ntiles == 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.ntiles + 1));  // (+ the union's)
  if (p.has_diffs)
    hipLaunchKernelGGL(kd_count_diffs_kernel, grid, dim3(KDB), 0, st, p);
  else
    hipLaunchKernelGGL(kd_count_kernel, grid, dim3(KDB), 0, st, p);
  return hipGetLastError();
}

}  // namespace dg
