// dg_kdcount.h — what the per-key count kernels share: kd_count_kernel (kdelta.hip, one keyed
// delta) and kk_count_kernel (kkeyed.hip, the fold of k keyed deltas) each walk a key per thread
// in their own way, then put the key's leaf change into the tree (tree_put) and end in
// kd_count_tail: the workgroup's figures, and in the last workgroup to arrive the count block
// (KdCount, dg_launch.h) that the write (dg_kdw.h), kd_finish_kernel, the splice and the host read.
#pragma once
#include "dg_launch.h"
#include "dg_tree.h"

#ifndef KDSTAMP  // (kdelta.hip's DG_STAMPS build defines it ahead of this header)
#define KDSTAMP(th, k) \
  do {                 \
  } while (0)
#endif

namespace dg {

namespace {

constexpr int KDB = KD_BLOCK;  // keys per workgroup, one per thread
static_assert(KD_RUN <= 64, "a key's kept rows are a 64-bit mask per side");

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

// The workgroup's KD_NV figures of every thread's x: the sums of x[0 .. KD_NV - 1) and, of the
// flags x[KD_NV - 1], whether any thread has KD_BIG and KD_MOVED.  Thread q < KD_NV returns
// figure q.  (`red` is free again after the caller's next barrier.)
__device__ __forceinline__ u64 kd_block_figures(const u64 (&x)[KD_NV], u64 (&red)[KD_NV][KDB / WAVE]) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
#pragma unroll
  for (int q = 0; q < KD_NV; q++) {
    u64 y = x[q];
    if (q < KD_NV - 1) {
#pragma unroll
      for (int d = WAVE / 2; d >= 1; d >>= 1) y += __shfl_xor(y, d, WAVE);
    } else {
      y = (__ballot(x[q] & KD_BIG) ? KD_BIG : 0) | (__ballot(x[q] & KD_MOVED) ? KD_MOVED : 0);
    }
    if (lane == 0) red[q][w] = y;
  }
  __syncthreads();
  u64 sum = 0, any = 0;  // (both, then a select: no branch between the waves' words)
  const int q = tid < KD_NV ? tid : 0;
#pragma unroll
  for (int i = 0; i < KDB / WAVE; i++) {
    sum += red[q][i];
    any |= red[q][i];
  }
  return q < KD_NV - 1 ? sum : any;
}

// The end of a count kernel's key workgroup `blk` (of p.ntiles), every thread with its key's
// figures v (KD_NV, dg_launch.h): the workgroup's figures go to p.part, and the last workgroup
// to arrive sums all of them into the count block -- the totals and the guard word (KdCount;
// KC_CTX is the context union's).  bad(n_d), called by one thread with the sum of v[4], says
// whether the delta rows the keys account for fall short of the delta: a delta row whose key
// is outside the keyset (KD_BAD).
template <class Bad>
__device__ __forceinline__ void kd_count_tail(const KdArgs& p, u64 blk, const u64 (&v)[KD_NV], Bad bad) {
  __shared__ u64 red[KD_NV][KDB / WAVE];
  __shared__ u64 carry[KD_NV];
  __shared__ u32 s_last;
  const int tid = threadIdx.x;
  // the workgroup's figures handed to the last workgroup, which sums them all -- and to the
  // write's workgroups (dg_kdw.h), which sum the earlier workgroups' for their offsets
  // themselves: a scan here was ~3 more round trips on the call's critical path
  const u64 s = kd_block_figures(v, red);
  if (tid < KD_NV) st_sc1(p.part + blk * KD_NV + tid, s);
  __syncthreads();
  if (tid == 0) {
    wait_vmem();  // (the figures are this wave's stores: out before its arrival is counted, dg_tree.h)
    s_last = __hip_atomic_fetch_add(p.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.ntiles - 1;
    if (s_last) __hip_atomic_store(p.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  KDSTAMP(0, 6);
  if (!s_last) return;
  // ---- the last workgroup: the totals and the guard into the count block
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
  const u64 c = kd_block_figures(x, red);
  if (tid < KD_NV) carry[tid] = c;
  __syncthreads();
  if (tid == 0) {
    const u64 n_chg = carry[2];
    u64 g = carry[6] & KD_BIG;
    if (bad(carry[4])) g |= KD_BAD;
    if (n_chg > p.cap) g |= KD_CAP;  // the caller's changed-key buffer is too small
    p.d_counts[KC_EDIT] = carry[1];
    p.d_counts[KC_CHANGED] = n_chg;
    p.d_counts[KC_ROWS] = carry[3];
    p.d_counts[KC_GUARD] = g;
    p.d_counts[KC_MOVED] = (carry[6] & KD_MOVED) ? 1 : 0;
    p.d_counts[KC_TAKEN] = carry[0];
    p.d_counts[KC_DKEYS] = carry[5];
  }
  KDSTAMP(0, 7);
}

}  // namespace

}  // namespace dg
