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
// reads as its delta (the section "the keyed fold of k deltas" below).
//
// Roofline: each key costs two searches (~6 dependent loads of the state, a few of the
// delta) and reads its few rows twice (the second time from L2); a sync delta of 125k keys
// into a 12.5M-row state reads ~10 MB.  Latency-bound by the search chains, not by bytes.
#include "dg_ctxu.h"
#include "dg_hash.h"
#include "dg_launch.h"
#include "dg_tree.h"

namespace dg {

namespace {

constexpr int KDB = KD_BLOCK;  // keys per workgroup, one per thread
constexpr u32 KVT = 1024;      // VV tables in LDS cover node ids < KVT
static_assert(KD_RUN <= 64, "a key's kept rows are a 64-bit mask per side");

// Map.get(vv, node, 0) >= cnt through the LDS table (node ids < KVT), else a search
__device__ __forceinline__ bool vv_covers(const u64* tab, const Ctx& c, u32 n, u64 cnt) {
  if (n < KVT) return tab[n] >= cnt;
  return ctx_covers(c.node, c.cnt, c.n, 0, n, cnt);
}

// first row of key k in s (lower bound) and its run, at most KD_RUN + 1 counted (4 rows a
// round trip, every load issued together at a clamped index)
__device__ __forceinline__ void key_run(const u64* key, u64 n, u64 k, u64& lo, u32& run) {
  lo = interp_lower_bound(key, 0, n, k);
  u64 e = lo;
  while (e < n) {
    u64 kk[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u64 v = key[e + q < n ? e + q : lo];
      kk[q] = e + q < n ? v : k + 1;
    }
    u32 c = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) c += (c == (u32)q && kk[q] == k) ? 1u : 0u;
    e += c;
    if (c < 4 || e - lo > KD_RUN) break;
  }
  run = (u32)(e - lo);
}

// MerkleMap.put/delete of the changed keys (the caller zeroed dirty and cdelta): key u's
// leaf change d and row-count change dr.  The keys are ascending, so a wave's keys of one
// bucket (and of one chunk) are adjacent lanes: segmented sums over the lanes (seg_incl,
// dg_tree.h) leave ONE atomic per bucket and per chunk.  merkle_build.hip's kd_tree_kernel
// applies the same with the opposite sign to undo it.
__device__ __forceinline__ void tree_put(const KdArgs& p, bool valid, u64 x, bool chg, u64 d, int dr) {
  const MerkleT& t = p.t;
  const int lane = threadIdx.x & (WAVE - 1);
  const u32 L1 = t.depth < MERKLE_UPL ? t.depth : MERKLE_UPL;
  bool bad = false, over = false;
  int act = 0;
  // (bucket_of, dg_tree.h, spelled out: through the helper the compiler places one scalar
  // instruction of the count kernels on the other side of a wait)
  const u64 b = valid ? (x << t.sb) >> (64 - t.depth) : ~0ull;
  if (valid && chg && (d != 0 || dr != 0)) {
    if (t.sb && (x >> (64 - t.sb)) != t.shard)
      bad = true;  // (skipped both ways)
    else
      act = 1;
  }
  if (!act) {
    d = 0;
    dr = 0;
  }
  const u64 c = b == ~0ull ? ~0ull : b >> L1;
  const u64 sd = seg_incl<u64>(d, b, lane);
  const int sr = seg_incl<int>(dr, b, lane), sa = seg_incl<int>(act, b, lane);
  const int cr = seg_incl<int>(dr, c, lane), ca = seg_incl<int>(act, c, lane);
  const u64 nb = __shfl_down(b, 1, WAVE), nc = __shfl_down(c, 1, WAVE);
  const bool last = lane == WAVE - 1;
  if (b != ~0ull && (last || nb != b) && sa) {  // the bucket's last lane: its node and row count
    u64* lvl = t.nodes + ((1ull << t.depth) - 1);
    atomicAdd((unsigned long long*)&lvl[b], (unsigned long long)sd);
    if (sr) {  // (its aligned 32-bit word of two u16 counts, as merkle_update_kernel)
      u32* wd = (u32*)t.counts + (b >> 1);
      const u32 sh = 16u * (u32)(b & 1);
      if (sr > 0) {
        const u32 old = atomicAdd(wd, (u32)sr << sh);
        over = ((old >> sh) & 0xFFFFu) + (u32)sr > 0xFFFFu;
      } else {
        atomicSub(wd, (u32)(-sr) << sh);
      }
    }
  }
  if (c != ~0ull && (last || nc != c) && ca) {  // the chunk's last lane: dirty, its row-count change
    p.dirty[c] = 1u;
    if (t.starts && cr) atomicAdd((unsigned long long*)&p.cdelta[c], (unsigned long long)(i64)cr);
  }
  if (__ballot(bad) && lane == 0) atomicOr(p.err, MERKLE_ERR_SHARD);
  if (__ballot(over) && lane == 0) atomicOr(p.err, MERKLE_ERR_COUNT);
}

// ---------------------------------------------------------------- count (+ scan)
// The workgroup's keys are ascending, so their delta rows are one contiguous range: two
// searches find its ends and its keys are staged in LDS (every key's delta run is found
// there, not by a search of the delta in memory).  (Narrowing the state searches to the
// workgroup's range the same way, by 64-ary wave searches, measured slower: 52 against
// 45 us at config 4 -- their 256 scattered lines per bound outweigh what each key saves.)
constexpr u32 KDL = 2048;  // delta keys staged per workgroup (more: searched in memory)
#ifdef DG_STAMPS
// Diagnostic build only (DG_STAMPS=1): per-workgroup timestamps (s_memrealtime, 100 MHz) of
// the count kernel, read back with dg_debug_kd_stamps (tools/kd_stamps.py).  No barriers
// added: thread `th` stamps slot k when it passes that point.
__device__ u64 g_kd_stamps[4096 * 8];
#define KDSTAMP(th, k)                                                        \
  do {                                                                        \
    if (threadIdx.x == (th) && blk < 4096)                                    \
      g_kd_stamps[blk * 8 + (k)] = __builtin_amdgcn_s_memrealtime();          \
  } while (0)
#else
#define KDSTAMP(th, k) \
  do {                 \
  } while (0)
#endif
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
  __shared__ u64 red[KD_NV][KDB / WAVE];
  __shared__ u32 s_last;
  __shared__ u32 s_cw[KDB / WAVE + 1];
  if (blockIdx.x == 0) {
    // Dots.union(state context, delta context) (:155) into the union scratch and
    // d_counts[KC_CTX], by a workgroup of its own beside the keys' (it needs only the inputs;
    // in the last workgroup's tail it added ~5 us to every call)
    ctx_union_block<KDB>(make_cu(p.ca, p.cd, p.uc_node, p.uc_cnt, p.d_counts + KC_CTX, p.cu_tmp), s_cw);
    return;
  }
  const u64 blk = blockIdx.x - 1;  // the keys' workgroups: 1 .. ntiles
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
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
    key_run(p.a.key, p.a.n, k, a_lo, na);  // the state: an interpolation search
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
      key_run(p.d.key, p.d.n, k, d_lo, nd);
    }
    big = na > KD_RUN || nd > KD_RUN;
  }
#ifndef DG_KD_EXP
#define DG_KD_EXP 0  // experiment builds only: 1 no row hashes, 2 no per-key join (wrong results)
#endif
  if (u < p.nk && !big && DG_KD_EXP < 2) {
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
          if (p.has_tree && DG_KD_EXP == 0) dh -= rh_row(p.t.th, ra);
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
          if (p.has_tree && DG_KD_EXP == 0) dh += rh_row(p.t.th, rb);
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
    p.runs[u] = big ? 0ull : (na | ((u64)nd << 16) | ((u64)ne << 32) | (chg ? 1ull << 48 : 0ull));
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
  // and stays in place.  (kk_count_body below flags every key of several rows that loses one
  // and gains one: wider, and as safe.)
  const bool moved = ne != na || back;
  v[6] = (big ? KD_BIG : 0u) | (moved ? KD_MOVED : 0u);
#pragma unroll
  for (int q = 0; q < KD_NV; q++) {
    u64 x = v[q];
    if (q < KD_NV - 1) {
#pragma unroll
      for (int d = WAVE / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d, WAVE);
    } else {
      x = __ballot(x & KD_BIG) ? KD_BIG : 0;
      x |= __ballot(v[q] & KD_MOVED) ? KD_MOVED : 0;
    }
    if (lane == 0) red[q][w] = x;
  }
  __syncthreads();
  // the workgroup's figures handed to the last workgroup, which scans them all
  if (tid < KD_NV) {
    u64 s = 0;
#pragma unroll
    for (int x = 0; x < KDB / WAVE; x++) s = tid < KD_NV - 1 ? s + red[tid][x] : (s | red[tid][x]);
    st_sc1(p.part + blk * KD_NV + tid, s);
  }
  __syncthreads();
  if (tid == 0) {
    wait_vmem();
    s_last = __hip_atomic_fetch_add(p.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.ntiles - 1;
    if (s_last) __hip_atomic_store(p.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  KDSTAMP(0, 6);
  if (!s_last) return;
  // ---- the last workgroup: the totals and the guard into the count block (KdCount,
  // dg_launch.h; KC_CTX is the context union's).  (The per-workgroup offsets are summed by
  // the write's workgroups themselves, dg_kdw.h: a scan here was ~3 more round trips on the
  // call's critical path.)
  __shared__ u64 carry[KD_NV];
  {
    u64 x[KD_NV];
#pragma unroll
    for (int q = 0; q < KD_NV; q++) x[q] = 0;
    for (u64 t = tid; t < p.ntiles; t += KDB) {  // (every load of a round issued together)
      u64 y[KD_NV];
#pragma unroll
      for (int q = 0; q < KD_NV; q++) y[q] = ld_sc1(p.part + t * KD_NV + q);
#pragma unroll
      for (int q = 0; q < KD_NV; q++) x[q] = q < KD_NV - 1 ? x[q] + y[q] : (x[q] | y[q]);
    }
#pragma unroll
    for (int q = 0; q < KD_NV; q++) {
      if (q < KD_NV - 1) {
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) x[q] += __shfl_xor(x[q], d, WAVE);
      } else {
        x[q] = (__ballot(x[q] & KD_BIG) ? KD_BIG : 0) | (__ballot(x[q] & KD_MOVED) ? KD_MOVED : 0);
      }
      if (lane == 0) red[q][w] = x[q];
    }
    __syncthreads();
    if (tid < KD_NV) {
      u64 c = 0;
#pragma unroll
      for (int i = 0; i < KDB / WAVE; i++) c = tid < KD_NV - 1 ? c + red[tid][i] : (c | red[tid][i]);
      carry[tid] = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const u64 n_ak = carry[0], n_e = carry[1], n_chg = carry[2], n_rows = carry[3], n_d = carry[4];
    u64 g = carry[6] & KD_BIG;
    if (n_d != p.d.n) g |= KD_BAD;      // a delta row whose key is outside the keyset
    if (n_chg > p.cap) g |= KD_CAP;     // the caller's changed-key buffer is too small
    p.d_counts[KC_EDIT] = n_e;
    p.d_counts[KC_CHANGED] = n_chg;
    p.d_counts[KC_ROWS] = n_rows;
    p.d_counts[KC_GUARD] = g;
    p.d_counts[KC_MOVED] = (carry[6] & KD_MOVED) ? 1 : 0;
    p.d_counts[KC_TAKEN] = n_ak;
    p.d_counts[KC_DKEYS] = carry[5];
  }
  KDSTAMP(0, 7);
}

__global__ __launch_bounds__(KDB) void kd_count_kernel(KdArgs p) { kd_count_body<false>(p); }
__global__ __launch_bounds__(KDB) void kd_count_diffs_kernel(KdArgs p) { kd_count_body<true>(p); }

// ---------------------------------------------------------------- the keyed fold of k deltas
// dg_join_deltas_keyed: kfold.hip's rule, evaluated by a thread per key of the keysets' union
// instead of a workgroup per bucket of the whole state.  For a batch whose every delta row
// has its key in its own delta's keyset the rule per candidate tuple r of key x is
//
//   for i ascending with x ∈ K_i:   P = P ? (r ∈ D_i || dot(r) ∉ c_i)
//                                         : (r ∈ D_i && dot(r) ∉ C_{i-1})
//
// with P = "r is a state row" at the start.  A thread walks its key's candidates in tuple
// order -- a merge of the key's state run with its run in every delta whose mask bit is set --
// so a tuple held by several deltas is ONE candidate whose holders are the bits M.  State rows
// give amask; the surviving new rows go, in tuple order, to the edit store E, and the per-key
// arrays are filled as kd_count_kernel fills them with d = E: kd_finish_kernel and
// splice_kernel then write the state exactly as they do for one delta.
//
// Per thread in LDS: each delta run's first row, length and cursor (a key may be in all 64
// keysets; 64 cursors do not fit registers), lane-major so that a wave's accesses to one
// delta's words fall on distinct banks.

// The VV tables and C_k: kfold_prep for VV contexts, as a launch of its own (one workgroup of
// KNT threads; tabC and tabP zeroed by the caller).
__global__ __launch_bounds__(KNT) void kk_prep_kernel(KkArgs q) {
  __shared__ u32 pres[KNT];
  __shared__ u32 wave[KNT / WAVE + 1];
  const u32 n = threadIdx.x;
  const int k = q.k;
  pres[n] = 0;
  __syncthreads();
  for (u64 e = n; e < q.c0.n; e += KNT) {
    const u32 nd = q.c0.node[e];
    if (nd >= (u32)KNT) {
      atomicOr(q.flag, KF_PREP_FAIL);
      continue;
    }
    q.tabP[nd] = q.c0.cnt[e];
    pres[nd] = 1;
  }
  for (int i = n / WAVE; i < k; i += KNT / WAVE) {  // one wave per delta context
    const Ctx c = q.runs[i].ctx;
    for (u64 e = n % WAVE; e < c.n; e += WAVE) {
      const u32 nd = c.node[e];
      if (nd >= (u32)KNT) {
        atomicOr(q.flag, KF_PREP_FAIL);
        continue;
      }
      q.tabC[(u64)i * KNT + nd] = c.cnt[e];
      pres[nd] = 1;
    }
  }
  __syncthreads();
  // prefix unions: C_i = C_{i-1} ⊔ c_i, per node the max (absent = 0); as in kfold_prep the
  // loads are batched ahead of the stores they would otherwise be ordered behind
  u64 acc = q.tabP[n];
  for (int i0 = 0; i0 < k; i0 += 8) {
    u64 c[8];
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = q.tabC[(u64)(i0 + j < k ? i0 + j : i0) * KNT + n];
    asm volatile("" ::: "memory");  // (all eight issued before any is used)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      acc = max(acc, i0 + j < k ? c[j] : 0ull);
      if (i0 + j + 1 < k) q.tabP[(u64)(i0 + j + 1) * KNT + n] = acc;
    }
  }
  u32 tot;
  const u32 pos = block_excl_scan<KNT>(pres[n], wave, &tot);  // C_k in node order
  if (pres[n]) {
    q.kd.uc_node[pos] = n;
    q.kd.uc_cnt[pos] = acc;
  }
  if (n == 0) q.kd.d_counts[KC_CTX] = tot;
}

__device__ __forceinline__ u64 kk_vv_at(const u64* tab, u32 i, u32 node) {
  return node < (u32)KNT ? tab[(u64)i * KNT + node] : 0ull;
}

struct KkRun {  // delta i's columns, staged per workgroup
  const u64 *key, *val, *cnt;
  const i64* ts;
  const u32* node;
  u64 n;
};

template <bool DIFFS>
__device__ __forceinline__ void kk_count_body(const KkArgs& q) {
  const KdArgs& p = q.kd;
  __shared__ KkRun s_run[KFOLD_MAX_K];
  __shared__ u32 s_lo[KFOLD_MAX_K][KDB];            // the key's first row in delta i
  __shared__ unsigned char s_nd[KFOLD_MAX_K][KDB];  // its rows there (<= KD_RUN), and how many
  __shared__ unsigned char s_cur[KFOLD_MAX_K][KDB]; //   of them the walk has passed
  __shared__ u64 red[KD_NV][KDB / WAVE];
  __shared__ u32 s_last;
  __shared__ u64 carry[KD_NV];
  const u64 blk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const u64 u = blk * KDB + tid;
  if (tid < q.k) {
    const Rows& R = q.runs[tid].rows;
    s_run[tid] = KkRun{R.key, R.val, R.cnt, R.ts, R.node, R.n};
  }
  u64 v[KD_NV] = {0, 0, 0, 0, 0, 0, 0};
  u64 a_lo = 0, am = 0, dh = 0, k = 0, msk = 0;
  u32 na = 0, nn = 0, ne = 0, nsum = 0;
  bool chg = false, big = false, removed = false;
  u64 ov = 0, nv = 0;    // (DIFFS) the old and the new winner's value id (no row: 0) ...
  i64 ots = 0, nts = 0;  // ... and ts
  if (u < p.nk) {
    k = p.keys[u];
    msk = q.masks[u];
    key_run(p.a.key, p.a.n, k, a_lo, na);
    big = na > KD_RUN;
  }
  __syncthreads();  // (the staged runs)
  // the key's run in every delta whose keyset holds it
  for (u64 b = msk; b; b &= b - 1) {
    const u32 i = (u32)__builtin_ctzll(b);
    u64 lo;
    u32 n;
    key_run(s_run[i].key, s_run[i].n, k, lo, n);
    big |= n > KD_RUN;
    s_lo[i][tid] = (u32)lo;
    s_nd[i][tid] = (unsigned char)(n > KD_RUN ? KD_RUN : n);
    s_cur[i][tid] = 0;
    nsum += n;
  }
  // the key's place in E: room for every delta row of the key (its new rows are at most as
  // many); one bump of the pointer per wave.  Σ over the keys <= Σ deltas[i].n = e_rows: a
  // delta's runs of distinct keys are disjoint.
  const u32 room = big ? 0u : nsum;
  const u32 incl = wave_incl_scan(room);
  u64 base = 0;
  if (lane == WAVE - 1 && incl) base = atomicAdd((unsigned long long*)q.e_next, (unsigned long long)incl);
  base = __shfl(base, WAVE - 1, WAVE);
  const u64 e_lo = base + incl - room;
  if (e_lo + room > q.e_rows) big = true;  // (never: the bound above; no store past E either way)
  if (u < p.nk && !big) {
    u32 i_s = 0, ncand = 0;
    Row ra{};
    if (na) ra = load_row(p.a, a_lo);
    while (true) {
      // the least tuple at the head of a delta run, and the deltas holding it
      bool have = false;
      Row mn{};
      u64 M = 0;
      for (u64 b = msk; b; b &= b - 1) {
        const u32 i = (u32)__builtin_ctzll(b);
        const u32 c = s_cur[i][tid];
        if (c >= s_nd[i][tid]) continue;
        const KkRun& R = s_run[i];
        const u64 j = (u64)s_lo[i][tid] + c;
        const Row r{k, R.val[j], R.cnt[j], R.ts[j], R.node[j]};
        bool lt = true, eq = false;
        if (have) row_cmp_bf(r, mn, lt, eq);
        if (eq) {
          M |= 1ull << i;
        } else if (lt) {
          mn = r;
          M = 1ull << i;
          have = true;
        }
      }
      if (!have && i_s >= na) break;
      int c;  // -1: the state row first, 1: the delta tuple first, 0: the same tuple
      if (i_s >= na) {
        c = 1;
      } else if (!have) {
        c = -1;
      } else {
        bool lt, eq;
        row_cmp_bf(ra, mn, lt, eq);
        c = eq ? 0 : (lt ? -1 : 1);
      }
      const Row r = c <= 0 ? ra : mn;
      const u64 Mc = c >= 0 ? M : 0ull;
      if (c >= 0) {  // the holders move on; a distinct delta tuple more
        for (u64 b = M; b; b &= b - 1) s_cur[__builtin_ctzll(b)][tid]++;
        if (++ncand > KD_RUN) {
          big = true;
          break;
        }
      }
      bool P = c <= 0;
      for (u64 b = msk; b; b &= b - 1) {
        const u32 i = (u32)__builtin_ctzll(b);
        const bool inD = (Mc >> i) & 1;
        const u64 ci = kk_vv_at(q.tabC, i, r.node), pi = kk_vv_at(q.tabP, i, r.node);
        P = P ? (inD || ci < r.cnt) : (inD && pi < r.cnt);
      }
      if (c <= 0) {  // a state row: kept or removed
        if (DIFFS) {
          const bool wo = (i_s == 0) | (ra.ts > ots);
          ots = wo ? ra.ts : ots;
          ov = wo ? ra.val : ov;
        }
        if (P) {
          am |= 1ull << i_s;
        } else {
          chg = removed = true;
          if (p.has_tree) dh -= rh_row(p.t.th, ra);
        }
        if (++i_s < na) ra = load_row(p.a, a_lo + i_s);
      } else if (P) {  // a new row: the next of the key's rows in E
        store_row(q.e, e_lo + nn, r);
        nn++;
        chg = true;
        if (p.has_tree) dh += rh_row(p.t.th, r);
      }
      if (P) {
        if (DIFFS) {
          const bool wn = (ne == 0) | (r.ts > nts);
          nts = wn ? r.ts : nts;
          nv = wn ? r.val : nv;
        }
        ne++;
      }
    }
  }
  if (u < p.nk && !big) {
    p.a_lo[u] = a_lo;
    p.d_lo[u] = e_lo;
    p.amask[u] = am;
    p.dmask[u] = nn >= 64 ? ~0ull : (1ull << nn) - 1;
    if (DIFFS) {
      p.dv_old[u] = ov;
      p.dv_new[u] = nv;
    }
  }
  if (big) {  // (no change recorded, so the undo skips the key too)
    chg = false;
    ne = na;
    nn = 0;
    dh = 0;
  }
  if (u < p.nk) {
    p.runs[u] = big ? 0ull : (na | ((u64)nn << 16) | ((u64)ne << 32) | (chg ? 1ull << 48 : 0ull));
    p.dh[u] = dh;
  }
  if (p.has_tree) tree_put(p, u < p.nk, k, chg, dh, (int)ne - (int)na);
  // the per-workgroup figures and the count block, as kd_count_kernel's.  Rows move whenever a
  // key's row count changes, and also when a key of several state rows loses one and gains
  // one: dg_kdw.h's in-place write would read back a row it has just written.
  const bool moved = ne != na || (na > 1 && removed && nn > 0);
  v[0] = big ? 0 : na;
  v[1] = big ? 0 : ne;
  v[2] = chg ? 1 : 0;
  v[3] = chg ? ne : 0;
  v[4] = nsum;
  v[5] = (u64)(i64)((int)(ne > 0) - (int)(na > 0));
  v[6] = (big ? KD_BIG : 0u) | (moved ? KD_MOVED : 0u);
#pragma unroll
  for (int x = 0; x < KD_NV; x++) {
    u64 y = v[x];
    if (x < KD_NV - 1) {
#pragma unroll
      for (int d = WAVE / 2; d >= 1; d >>= 1) y += __shfl_xor(y, d, WAVE);
    } else {
      y = (__ballot(v[x] & KD_BIG) ? KD_BIG : 0) | (__ballot(v[x] & KD_MOVED) ? KD_MOVED : 0);
    }
    if (lane == 0) red[x][w] = y;
  }
  __syncthreads();
  if (tid < KD_NV) {
    u64 s = 0;
#pragma unroll
    for (int x = 0; x < KDB / WAVE; x++) s = tid < KD_NV - 1 ? s + red[tid][x] : (s | red[tid][x]);
    st_sc1(p.part + blk * KD_NV + tid, s);
  }
  __syncthreads();
  if (tid == 0) {
    wait_vmem();
    s_last = __hip_atomic_fetch_add(p.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.ntiles - 1;
    if (s_last) __hip_atomic_store(p.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  // ---- the last workgroup: the totals and the guard into the count block
  {
    u64 x[KD_NV];
#pragma unroll
    for (int z = 0; z < KD_NV; z++) x[z] = 0;
    for (u64 t = tid; t < p.ntiles; t += KDB) {
      u64 y[KD_NV];
#pragma unroll
      for (int z = 0; z < KD_NV; z++) y[z] = ld_sc1(p.part + t * KD_NV + z);
#pragma unroll
      for (int z = 0; z < KD_NV; z++) x[z] = z < KD_NV - 1 ? x[z] + y[z] : (x[z] | y[z]);
    }
#pragma unroll
    for (int z = 0; z < KD_NV; z++) {
      if (z < KD_NV - 1) {
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) x[z] += __shfl_xor(x[z], d, WAVE);
      } else {
        x[z] = (__ballot(x[z] & KD_BIG) ? KD_BIG : 0) | (__ballot(x[z] & KD_MOVED) ? KD_MOVED : 0);
      }
      if (lane == 0) red[z][w] = x[z];
    }
    __syncthreads();
    if (tid < KD_NV) {
      u64 c = 0;
#pragma unroll
      for (int i = 0; i < KDB / WAVE; i++) c = tid < KD_NV - 1 ? c + red[tid][i] : (c | red[tid][i]);
      carry[tid] = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const u64 n_chg = carry[2];
    u64 g = carry[6] & KD_BIG;
    // a delta row whose key is outside its delta's keyset: the keys' runs do not add up to the
    // deltas' rows; a node id the VV tables do not hold
    if (carry[4] != q.e_rows || (*q.flag & KF_PREP_FAIL)) g |= KD_BAD;
    if (n_chg > p.cap) g |= KD_CAP;
    p.d_counts[KC_EDIT] = carry[1];
    p.d_counts[KC_CHANGED] = n_chg;
    p.d_counts[KC_ROWS] = carry[3];
    p.d_counts[KC_GUARD] = g;
    p.d_counts[KC_MOVED] = (carry[6] & KD_MOVED) ? 1 : 0;
    p.d_counts[KC_TAKEN] = carry[0];
    p.d_counts[KC_DKEYS] = carry[5];
  }
}

__global__ __launch_bounds__(KDB) void kk_count_kernel(KkArgs q) { kk_count_body<false>(q); }
__global__ __launch_bounds__(KDB) void kk_count_diffs_kernel(KkArgs q) { kk_count_body<true>(q); }

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

hipError_t launch_kk_join(const KkArgs& q0, hipStream_t st) {
  KkArgs q = q0;
  q.kd.ntiles = (q.kd.nk + KDB - 1) / KDB;
  if (q.kd.ntiles == 0 || q.k < 1 || q.k > KFOLD_MAX_K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kk_prep_kernel, dim3(1), dim3(KNT), 0, st, q);
  const dim3 grid((unsigned)q.kd.ntiles);
  if (q.kd.has_diffs)
    hipLaunchKernelGGL(kk_count_diffs_kernel, grid, dim3(KDB), 0, st, q);
  else
    hipLaunchKernelGGL(kk_count_kernel, grid, dim3(KDB), 0, st, q);
  return hipGetLastError();
}

}  // namespace dg
