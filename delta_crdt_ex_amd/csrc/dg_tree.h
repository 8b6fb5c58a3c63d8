// dg_tree.h — the device side of the Merkle tree (dg_merkle, include/deltagpu.h): what
// the tree kernels (merkle_build.hip, merkle_diff.hip, merkle_cont.hip), the keyed delta
// join (kdelta.hip, kkeyed.hip) and the fused small-delta join (small.hip) share.
//
// Tree (MerkleT, dg_launch.h): the keys whose top `sb` bits equal `shard` (a key-hash shard,
// SURVEY §8(e); sb = 0 covers every key) in 2^depth buckets by the next `depth` bits.
// Key ids are 64-bit hashes, so a bucket is a contiguous row range of the sorted
// store, and the tree keeps NO per-key leaves: the bucket hash is Σ row_hash over the
// bucket's rows (mod 2^64, order-free), a key's leaf Σ row_hash over its rows is
// recomputed from the store where a diff needs it.  Level `depth` holds the buckets,
// parent = node_hash(left, right).  Because node_hash does not depend on position,
// the shard trees of a 2^sb-way split are exactly the level-sb subtrees of the
// unsharded tree (dg_merkle_fold_roots recombines them).
//
// Row hashes cover term hashes of the value and node when the tree carries them
// (dg_term_hashes: trees then compare across interning tables and BEAM nodes), the ids
// otherwise.  The tree also keeps each bucket's row count (u16), maintained by build and
// update, read by the diff.
#pragma once
#include "dg_hash.h"
#include "dg_launch.h"

namespace dg {

constexpr u32 ERR_SHARD = MERKLE_ERR_SHARD, ERR_COUNT = MERKLE_ERR_COUNT;  // input-error bits

inline unsigned grid_of(u64 n, int b) { return (unsigned)((n + b - 1) / b); }

// ---------------------------------------------------------------- row hashes
// The value's and the node's terms in a row hash (dg_term_hashes): a canonical integer
// value id [2^58, 2^63) and ids missing from the tables stand for themselves.
__device__ __forceinline__ u64 th_val(const TermH& th, u64 v) {
  if (!th.on || th.nv == 0 || (v >= (1ull << 58) && v < (1ull << 63))) return v;
  u64 lo = 0, hi = th.nv;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (th.vid[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < th.nv && th.vid[lo] == v) ? th.vh[lo] : v;
}

__device__ __forceinline__ u64 th_node(const TermH& th, u32 n) {
  return (th.on && (u64)n < th.nn) ? th.nh[n] : (u64)n;
}

// of a row in registers / of row i of a store
__device__ __forceinline__ u64 rh_row(const TermH& th, const Row& r) {
  return row_hash(r.key, th_val(th, r.val), r.ts, th_node(th, r.node), r.cnt);
}
__device__ __forceinline__ u64 rh(const Rows& s, u64 i, const TermH& th) {
  return row_hash(s.key[i], th_val(th, s.val[i]), s.ts[i], th_node(th, s.node[i]), s.cnt[i]);
}

// ---------------------------------------------------------------- buckets
__device__ __forceinline__ u64 bucket_of(const MerkleT& t, u64 key) {
  return (key << t.sb) >> (64 - t.depth);
}

// First index of `keys[0, n)` (ascending) at or after bucket b's first key; b may be
// 2^depth (the end of the tree's key range).
__device__ __forceinline__ u64 bucket_start(const MerkleT& t, const u64* keys, u64 n, u64 b) {
  const u32 sh = 64 - t.sb - t.depth;  // >= 20
  if (b >> t.depth) {                  // past the last bucket
    if (t.sb == 0 || t.shard == (1ull << t.sb) - 1) return n;
    return lower_bound(keys, 0, n, (t.shard + 1) << (64 - t.sb));
  }
  const u64 base = t.sb ? (t.shard << (64 - t.sb)) : 0ull;
  return lower_bound(keys, 0, n, base + (b << sh));
}

// The same by one wave (wave_lower_bound): every lane returns the same value.
__device__ __forceinline__ u64 wave_bucket_start(const MerkleT& t, const u64* keys, u64 n, u64 b) {
  if (b >> t.depth) {
    if (t.sb == 0 || t.shard == (1ull << t.sb) - 1) return n;
    return wave_lower_bound(keys, n, (t.shard + 1) << (64 - t.sb));
  }
  const u64 base = t.sb ? (t.shard << (64 - t.sb)) : 0ull;
  return wave_lower_bound(keys, n, base + (b << (64 - t.sb - t.depth)));
}

// ---------------------------------------------------------------- key-level merge
// Merge keys[ia, ie) of store A (rows) with B, where B is either a store (rows) or a
// list of (key, leaf) pairs; emit the keys present on one side only or with different
// leaves.  WRITE: store them at out[o..) (only below cap); returns the count.
// LOC (the full diff's take form): each emitted key's run in the chosen store (side 0: A,
// 1: B) is known here as the walk's start and end, so it goes to loc[o..) beside the key
// as row | length << DIFF_LOC_LEN (length 0: the store lacks the key) and its length is added to
// *nrows -- the key is never searched for again.
template <bool B_LEAVES, bool WRITE, bool LOC>
__device__ __forceinline__ u32 merge_bucket_impl(const Rows& A, const TermH& tha, u64 ia, u64 ie, const Rows& B,
                                                 const TermH& thb, const u64* bk, const u64* bh, u64 jb,
                                                 u64 je, u64* out, u64 o, u64 cap, u64* loc, u32 side,
                                                 u32* nrows) {
  u32 c = 0;
  while (ia < ie || jb < je) {
    [[maybe_unused]] const u64 ia0 = ia, jb0 = jb;
    const u64 ka = ia < ie ? A.key[ia] : ~0ull;
    const u64 kb = jb < je ? (B_LEAVES ? bk[jb] : B.key[jb]) : ~0ull;
    const bool has_a = ia < ie && (jb >= je || ka <= kb);
    const bool has_b = jb < je && (ia >= ie || kb <= ka);
    const u64 k = has_a ? ka : kb;
    u64 ha = 0, hb = 0;
    if (has_a)
      for (; ia < ie && A.key[ia] == k; ia++) ha += rh(A, ia, tha);
    if (has_b) {
      if (B_LEAVES) {
        hb = bh[jb++];
      } else {
        for (; jb < je && B.key[jb] == k; jb++) hb += rh(B, jb, thb);
      }
    }
    if (!(has_a && has_b) || ha != hb) {
      if (WRITE && o + c < cap) out[o + c] = k;
      if constexpr (LOC) {
        const u64 len = side ? jb - jb0 : ia - ia0;
        if (WRITE && o + c < cap) loc[o + c] = (side ? jb0 : ia0) | (len << DIFF_LOC_LEN);
        if (nrows) *nrows += (u32)len;
      }
      c++;
    }
  }
  return c;
}

template <bool B_LEAVES, bool WRITE>
__device__ u32 merge_bucket(const Rows& A, const TermH& tha, u64 ia, u64 ie, const Rows& B,
                            const TermH& thb, const u64* bk, const u64* bh, u64 jb, u64 je,
                            u64* out, u64 o, u64 cap) {
  return merge_bucket_impl<B_LEAVES, WRITE, false>(A, tha, ia, ie, B, thb, bk, bh, jb, je, out, o, cap, nullptr, 0,
                                                   nullptr);
}

// two stores, every key written (the full diff's global path)
template <bool WRITE>
__device__ u32 merge_bucket_loc(const Rows& A, const TermH& tha, u64 ia, u64 ie, const Rows& B,
                                const TermH& thb, u64 jb, u64 je, u64* out, u64 o, u64* loc, u32 side,
                                u32* nrows) {
  return merge_bucket_impl<false, WRITE, true>(A, tha, ia, ie, B, thb, nullptr, nullptr, jb, je, out, o, ~0ull, loc,
                                               side, nrows);
}

// ---------------------------------------------------------------- hand-offs
// Agent-scope (write-through, sc1) stores and loads of the words one workgroup hands to
// the last one to arrive, and the wait for a lane's own stores before it arrives
// (MI355X_MICROARCH.md "Valid forms", hand-off table row 1).
__device__ __forceinline__ void wait_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ void st_sc1(u64* p, u64 v) {
  __hip_atomic_store((__attribute__((address_space(1))) u64*)p, v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 ld_sc1(const u64* p) {
  return __hip_atomic_load((__attribute__((address_space(1))) u64*)p, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Inclusive sums over the wave's segments (contiguous runs of lanes with one `seg`): a
// wave's ascending keys of one bucket, or of one chunk, are adjacent lanes, so the put /
// delete of a batch of keys costs ONE atomic per bucket and per chunk (a small tree's few
// buckets took a thousand same-address atomics per word from a batch of mutations: 16 us
// for 1000 keys).
template <class T>
__device__ __forceinline__ T seg_incl(T v, u64 seg, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T y = __shfl_up(v, d, WAVE);
    const u64 sy = __shfl_up(seg, d, WAVE);
    if (lane >= d && sy == seg) v += y;
  }
  return v;
}

}  // namespace dg
