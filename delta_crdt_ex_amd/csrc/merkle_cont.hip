// merkle_cont.hip — the partial diff of two Merkle trees (dg_tree.h describes them):
// prepare_partial_diff / continue_partial_diff, 8 levels per message (reference
// lib/delta_crdt/causal_crdt.ex:96,255).
//
// Node-form continuations (positions + the sender's hashes at one level) are compared and
// expanded `levels` levels down; at the bucket level the reply is a leaf-form continuation
// (the sender's (key, leaf) pairs of the differing buckets), which the peer merges with its
// own rows into keys.  cont_hop_kernel does one whole hop of a small continuation in one
// workgroup (dg_merkle_continue_home), or k such hops in k workgroups (dg_merkle_continues), a
// leaf form's kept keys then with their rows where asked for (dg_merkle_continues_take).
#include <type_traits>

#include "dg_home.h"
#include "dg_launch.h"
#include "dg_tree.h"

namespace dg {

namespace {

// the exclusive scan of per-tile counts between a count and a write pass (one workgroup)
constexpr int DSB = 1024;
__global__ __launch_bounds__(DSB) void tile_scan_kernel(const u64* cnt, u64* off, u64 ntiles,
                                                        u64* d_count) {
  __shared__ u32 s_wave[DSB / WAVE + 1];
  __shared__ u64 s_carry;
  scan_tile_counts<DSB>(cnt, off, ntiles, d_count, s_wave, &s_carry);
}

// ---------------------------------------------------------------- partial diff
// Node form: entry i = (pos[i], hash[i]) at level L.  Flag the entries whose own node
// differs; count / scan / compact their positions.
constexpr int PB = 256;

__global__ __launch_bounds__(PB) void cont_count_kernel(MerkleT t, u32 L, const u64* pos, const u64* hash,
                                                        u64 n, u64* cnt) {
  __shared__ u32 s_wave[PB / WAVE + 1];
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  u32 d = 0;
  if (i < n) d = t.nodes[((1ull << L) - 1) + pos[i]] != hash[i] ? 1u : 0u;
  u32 tot;
  block_excl_scan<PB>(d, s_wave, &tot);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PB) void cont_compact_kernel(MerkleT t, u32 L, const u64* pos, const u64* hash,
                                                          u64 n, const u64* off, u64* dpos) {
  __shared__ u32 s_wave[PB / WAVE + 1];
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  u32 d = 0;
  if (i < n) d = t.nodes[((1ull << L) - 1) + pos[i]] != hash[i] ? 1u : 0u;
  u32 tot;
  const u32 ex = block_excl_scan<PB>(d, s_wave, &tot);
  if (d) dpos[off[blockIdx.x] + ex] = pos[i];
}

// Children at level L + k of the m differing positions: out entry j = child (j & (2^k-1))
// of dpos[j >> k], with this tree's hash.
__global__ __launch_bounds__(PB) void cont_expand_kernel(MerkleT t, u32 L, u32 k, const u64* dpos, u64 m,
                                                         u64* opos, u64* ohash) {
  const u64 j = (u64)blockIdx.x * PB + threadIdx.x;
  if (j >= (m << k)) return;
  const u64 p = (dpos[j >> k] << k) | (j & ((1ull << k) - 1));
  opos[j] = p;
  ohash[j] = t.nodes[((1ull << (L + k)) - 1) + p];
}

// prepare_partial_diff: every node of level L, positions and hashes (host or device)
__global__ __launch_bounds__(PB) void cont_prepare_kernel(MerkleT t, u32 L, u64* opos, u64* ohash) {
  const u64 j = (u64)blockIdx.x * PB + threadIdx.x;
  if (j >> L) return;
  opos[j] = j;
  ohash[j] = t.nodes[((1ull << L) - 1) + j];
}

// Leaf form, built by the side that found differing buckets: per bucket its distinct
// keys (count pass) and then (key, leaf) pairs at the bucket's offset (write pass).
template <bool WRITE>
__global__ __launch_bounds__(PB) void leaves_kernel(MerkleT t, Rows s, const u64* buckets, u64 nb,
                                                    u64* cnt, const u64* off, u64* ok, u64* oh) {
  __shared__ u32 s_wave[PB / WAVE + 1];
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  u64 r = 0, re = 0;
  u32 c = 0;
  if (i < nb) {
    r = bucket_start(t, s.key, s.n, buckets[i]);
    re = bucket_start(t, s.key, s.n, buckets[i] + 1);
    for (u64 x = r; x < re; x++) c += (x == r || s.key[x] != s.key[x - 1]) ? 1u : 0u;
  }
  u32 tot;
  const u32 ex = block_excl_scan<PB>(c, s_wave, &tot);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
    return;
  }
  u64 o = off[blockIdx.x] + ex;
  for (u64 x = r; x < re;) {
    const u64 k = s.key[x];
    u64 h = 0;
    for (; x < re && s.key[x] == k; x++) h += rh(s, x, t.th);
    ok[o] = k;
    oh[o++] = h;
  }
}

// Leaf form received: per listed bucket, merge the peer's (key, leaf) pairs with this
// store's rows of the bucket; count / write the differing keys.
template <bool WRITE>
__global__ __launch_bounds__(PB) void leafdiff_kernel(MerkleT t, Rows s, const u64* buckets, u64 nb,
                                                      const u64* pk, const u64* ph, u64 np, u64* cnt,
                                                      const u64* off, u64* out, u64 cap) {
  __shared__ u32 s_wave[PB / WAVE + 1];
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  u64 r = 0, re = 0, j = 0, je = 0;
  u32 c = 0;
  if (i < nb) {
    const u64 b = buckets[i];
    r = bucket_start(t, s.key, s.n, b);
    re = bucket_start(t, s.key, s.n, b + 1);
    j = bucket_start(t, pk, np, b);
    je = bucket_start(t, pk, np, b + 1);
    c = merge_bucket<true, false>(s, t.th, r, re, s, t.th, pk, ph, j, je, nullptr, 0, 0);
  }
  u32 tot;
  const u32 ex = block_excl_scan<PB>(c, s_wave, &tot);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
    return;
  }
  const u64 o = off[blockIdx.x] + ex;
  if (c && o < cap) merge_bucket<true, true>(s, t.th, r, re, s, t.th, pk, ph, j, je, out, o, cap);
}

__global__ void pairs_before_kernel(MerkleT t, const u64* keys, u64 n, const u64* bucket, u64* out) {
  if (threadIdx.x == 0) out[0] = bucket_start(t, keys, n, bucket[0]);
}

// ---------------------------------------------------------------- a small partial-diff hop
// dg_merkle_continue_home: one hop of continue_partial_diff (+ truncate_diff to `max`) for
// a continuation of at most CS_IN entries / CS_B buckets, by ONE workgroup, results written
// straight into the caller's (host) arrays, one host wait -- the general path is three
// to five launches, each waited for.  Same results as dg_merkle_continue followed by
// dg_merkle_truncate(max), except that capacity is asked of the truncated output only.
//   node form, level L < depth : compare, compact the differing positions (input order),
//                                expand by k levels, only the first `max` children made
//   node form, level == depth  : the first `max` differing buckets, their (key, leaf) pairs
//                                from the store (a bucket's rows: an interpolation search
//                                for its first key, the tree's row count for the rest)
//   leaf form                  : per bucket, the store's rows merged with the peer's pairs
//                                (staged in LDS): the differing keys, the first kcap written
// The result header goes to home[0..8) and the sequence number is published (dg_home.h).
constexpr int CSN = 512;  // threads (256 VGPRs: a bucket's 16 rows in registers)
constexpr u32 CS_PER = CS_IN / CSN;
static_assert(CS_IN % CSN == 0, "whole entries per thread");

__device__ __forceinline__ u64 bucket_first_key(const MerkleT& t, u64 b) {
  return (t.sb ? (t.shard << (64 - t.sb)) : 0ull) + (b << (64 - t.sb - t.depth));
}

// the store rows of bucket b: [r, r + counts[b]) (the tree describes the store), clamped
__device__ __forceinline__ void bucket_rows(const MerkleT& t, const Rows& s, u64 b, u64& r, u64& re) {
  r = interp_lower_bound(s.key, 0, s.n, bucket_first_key(t, b));
  re = min<u64>(r + t.counts[b], s.n);
}

// A bucket's (key, leaf) pairs in registers: its rows (at most BR; the tree's row count)
// loaded together -- one round trip after the search, two past BR / 2 rows -- hashed,
// and the runs of equal keys summed (head bit i: row i starts a key, leaf[i] its sum).
// big: more rows than that (the generic loops over global memory).
constexpr int BR = 16;
struct BucketPairs {
  u64 key[BR], leaf[BR];
  u32 head;
  bool big;
  u64 r, re;
};

__device__ __forceinline__ void bucket_pairs(const MerkleT& t, const Rows& s, u64 b, BucketPairs& o) {
  const u32 cnt = t.counts[b];
  const u64 r = interp_lower_bound(s.key, 0, s.n, bucket_first_key(t, b));
  const u64 re = min<u64>(r + cnt, s.n);
  o.r = r;
  o.re = re;
  o.big = re - r > (u64)BR;
  o.head = 0;
  if (o.big || re == r) return;
  const u32 m = (u32)(re - r);
  u64 hs[BR];
#pragma unroll
  for (int half = 0; half < 2; half++) {
    if (half == 1 && m <= (u32)(BR / 2)) {
#pragma unroll
      for (int i = BR / 2; i < BR; i++) {
        o.key[i] = 0;
        hs[i] = 0;
      }
      break;
    }
    u64 k[BR / 2], v[BR / 2], c[BR / 2];
    i64 ts[BR / 2];
    u32 nd[BR / 2];
#pragma unroll
    for (int q = 0; q < BR / 2; q++) {  // every load issued before any is used
      const int i = half * (BR / 2) + q;
      const u64 x = r + (u64)((u32)i < m ? i : m - 1);
      k[q] = s.key[x];
      v[q] = s.val[x];
      ts[q] = s.ts[x];
      nd[q] = s.node[x];
      c[q] = s.cnt[x];
    }
#pragma unroll
    for (int q = 0; q < BR / 2; q++) {
      const int i = half * (BR / 2) + q;
      o.key[i] = k[q];
      hs[i] = row_hash(k[q], th_val(t.th, v[q]), ts[q], th_node(t.th, nd[q]), c[q]);
    }
  }
  u64 acc = 0;
#pragma unroll
  for (int i = BR - 1; i >= 0; i--) {
    const bool valid = (u32)i < m;
    const bool cont = (u32)(i + 1) < m && o.key[i + 1 < BR ? i + 1 : i] == o.key[i];
    acc = valid ? hs[i] + (cont ? acc : 0ull) : 0ull;
    o.leaf[i] = acc;
    if (valid && (i == 0 || o.key[i > 0 ? i - 1 : 0] != o.key[i])) o.head |= 1u << i;
  }
}

// distinct keys of rows [r, re) / their (key, leaf) pairs at out[o..): over global memory
__device__ __forceinline__ u32 distinct_keys(const Rows& s, u64 r, u64 re) {
  u32 c = 0;
  for (u64 x = r; x < re; x++) c += (x == r || s.key[x] != s.key[x - 1]) ? 1u : 0u;
  return c;
}

__device__ __forceinline__ u32 pairs_global(const MerkleT& t, const Rows& s, u64 r, u64 re, u64* opos, u64* ohash,
                                            u64 o) {
  u32 c = 0;
  for (u64 x = r; x < re;) {
    const u64 key = s.key[x];
    u64 lf = 0;
    for (; x < re && s.key[x] == key; x++) lf += rh(s, x, t.th);
    opos[o + c] = key;
    ohash[o + c] = lf;
    c++;
  }
  return c;
}

// merge_bucket with the store side in registers: the keys on one side only or with
// different leaves, ascending (WRITE: out[o..), below cap)
template <bool WRITE>
__device__ __forceinline__ u32 merge_regs(const BucketPairs& bp, const u64* pk, const u64* ph, u64 j, u64 je,
                                          u64* out, u64 o, u64 cap) {
  u32 c = 0;
  auto emit = [&](u64 k) {
    if (WRITE && o + c < cap) out[o + c] = k;
    c++;
  };
#pragma unroll
  for (int i = 0; i < BR; i++) {
    if (!(bp.head >> i & 1u)) continue;
    const u64 k = bp.key[i];
    for (; j < je && pk[j] < k; j++) emit(pk[j]);
    if (j < je && pk[j] == k) {
      if (ph[j] != bp.leaf[i]) emit(k);
      j++;
    } else {
      emit(k);
    }
  }
  for (; j < je; j++) emit(pk[j]);
  return c;
}

// merge_bucket of the store's rows with the staged pairs.  INLINE: inlined at this call; the take
// form is large enough that the compiler would otherwise call it, with the hop's arguments and the
// tree passed through a stack frame (384 B of scratch)
template <bool WRITE, bool INLINE>
__device__ __forceinline__ u32 merge_big(const Rows& s, const TermH& th, u64 r, u64 re, const u64* pk, const u64* ph,
                                         u64 j, u64 je, u64* out, u64 o, u64 cap) {
  if constexpr (INLINE) {
    [[clang::always_inline]] return merge_bucket<true, WRITE>(s, th, r, re, s, th, pk, ph, j, je, out, o, cap);
  } else {
    return merge_bucket<true, WRITE>(s, th, r, re, s, th, pk, ph, j, je, out, o, cap);
  }
}

// dg_merkle_continues: the same hop by workgroup j of a grid of k <= CONT_BATCH_MAX, for hop j
// of a batch (cont_hop_kernel<true>; <false> is the single hop above, instruction for
// instruction; <true, true> is the take form below, the same hop and completion).  The tree,
// the store, `levels` and `max` are the launch's; hop j's numbers and pointers come from
// descriptor j (page-locked host memory, read through uniform loads), its result header goes
// to slot j of hdr (page-locked too).  No workgroup waits for another.
//
// Completion, and why the host that has seen `seq` sees every workgroup's writes:
//   (1) every thread of a workgroup, after its last write to host memory (outputs, keys, the
//       header; in the take form also the rows, their offsets and the row total, all written
//       by take_hop and its caller, before this point), executes __threadfence_system(): a
//       release fence at system scope -- the thread's earlier writes are performed with respect
//       to the host before anything the thread, or a thread that synchronizes with it, does
//       afterwards;
//   (2) the workgroup barrier orders all its threads' fences before lane 0's add to the
//       arrival word (agent scope: the adds of one launch are a total order on one word);
//   (3) the workgroup whose add returns gridDim.x - 1 has read, through the chain of
//       read-modify-writes, the adds of all the others, each of which follows that
//       workgroup's fences (2); its own __threadfence_system() after the add (acquire and
//       release) therefore orders every workgroup's host writes before its store of `seq`
//       (publish_counts: another system fence, then a system-scope release store);
//   (4) the host reads `seq` and then fences (wait_published), so it reads the headers and
//       the outputs after (3).
// The arrival word is zero between launches: the last workgroup, which alone knows that every
// add has happened, stores 0 before it publishes, and a launch that did not start added nothing.
//
// The kernel is the template and its LDS stays function-local: with the arrays gathered into
// one namespace-scope block, or with the single hop's arguments copied rather than bound by
// reference (hop_args), the single hop's code moved (188 VGPRs, another schedule); as it
// stands <false> is the former cont_small_kernel in every instruction and .amdhsa line.

// the hop's arguments: the call's own, or those of this workgroup's descriptor
__device__ __forceinline__ const ContSmallArgs& hop_args(const ContSmallArgs& p) { return p; }
__device__ __forceinline__ ContSmallArgs hop_args(const ContBatchArgs& p) {
  ContSmallArgs a;
  const ContHop& d = p.hops[blockIdx.x];
  a.s = p.s;
  a.level = d.level;
  a.levels = p.levels;
  a.max = p.max;
  a.ipos = d.ipos;
  a.ihash = d.ihash;
  a.ibucket = d.ibucket;
  a.n = d.n;
  a.nb = d.nb;
  a.opos = d.opos;
  a.ohash = d.ohash;
  a.obucket = d.obucket;
  a.ocap = d.ocap;
  a.ocap_b = d.ocap_b;
  a.keys = d.keys;
  a.kcap = d.kcap;
  a.home = p.hdr + (u64)blockIdx.x * CONT_HDR_STRIDE;
  return a;
}

// ---- the batch hop with take (dg_merkle_continues_take): a leaf form's kept keys and their rows
// The differing keys of one bucket in ascending order, each with its rows in the store:
// emit(key, first row, rows), no rows for a key only the peer holds.  walk_regs is merge_regs
// (a key's rows end at the next head bit), walk_global is merge_bucket over global memory.
template <class F>
__device__ __forceinline__ void walk_regs(const BucketPairs& bp, const u64* pk, const u64* ph, u64 j, u64 je,
                                          F emit) {
  const u32 m = (u32)(bp.re - bp.r);
#pragma unroll
  for (int i = 0; i < BR; i++) {
    if (!(bp.head >> i & 1u)) continue;
    const u64 k = bp.key[i];
    const u32 rest = bp.head >> (i + 1);
    const u32 n = (rest ? (u32)(i + 1) + (u32)__builtin_ctz(rest) : m) - (u32)i;
    for (; j < je && pk[j] < k; j++) emit(pk[j], 0ull, 0ull);
    if (j < je && pk[j] == k) {
      if (ph[j] != bp.leaf[i]) emit(k, bp.r + i, (u64)n);
      j++;
    } else {
      emit(k, bp.r + i, (u64)n);
    }
  }
  for (; j < je; j++) emit(pk[j], 0ull, 0ull);
}

// the same keys again without the leaves: `taken` has bit i where walk_regs emitted the key
// whose rows start at row i (a key only the peer holds is always emitted)
template <class F>
__device__ __forceinline__ void walk_taken(const BucketPairs& bp, u32 taken, const u64* pk, u64 j, u64 je, F emit) {
  const u32 m = (u32)(bp.re - bp.r);
#pragma unroll
  for (int i = 0; i < BR; i++) {
    if (!(bp.head >> i & 1u)) continue;
    const u64 k = bp.key[i];
    const u32 rest = bp.head >> (i + 1);
    const u32 n = (rest ? (u32)(i + 1) + (u32)__builtin_ctz(rest) : m) - (u32)i;
    for (; j < je && pk[j] < k; j++) emit(pk[j], 0ull, 0ull);
    if (j < je && pk[j] == k) j++;
    if (taken >> i & 1u) emit(k, bp.r + i, (u64)n);
  }
  for (; j < je; j++) emit(pk[j], 0ull, 0ull);
}

template <class F>
__device__ __forceinline__ void walk_global(const Rows& s, const TermH& th, u64 ia, u64 ie, const u64* pk,
                                            const u64* ph, u64 j, u64 je, F emit) {
  while (ia < ie || j < je) {
    const u64 ka = ia < ie ? s.key[ia] : ~0ull;
    const u64 kb = j < je ? pk[j] : ~0ull;
    const bool has_a = ia < ie && (j >= je || ka <= kb);
    const bool has_b = j < je && (ia >= ie || kb <= ka);
    const u64 k = has_a ? ka : kb;
    const u64 a0 = ia;
    u64 ha = 0, hb = 0;
    if (has_a)
      for (; ia < ie && s.key[ia] == k; ia++) ha += rh(s, ia, th);
    if (has_b) hb = ph[j++];
    if (!(has_a && has_b) || ha != hb) emit(k, a0, ia - a0);
  }
}

// One leaf-form hop's keys and rows by its workgroup: this thread's bucket holds the keys
// [ko, ko + c) of the hop's `tot`.  The keys below kcap are written as the plain hop writes
// them and their rows counted in the same walk; a block scan gives this thread's row offset;
// a second walk writes offs[] and, per CS_IN output rows, the rows' store indices into s_src
// (s_dpos: unused by the leaf form), from which the whole workgroup copies the five columns with
// consecutive lanes on consecutive rows -- whole lines to host memory, where a thread storing
// its own keys' rows would store 8 bytes at a time.  More rows than rcap: only the total is
// returned (nothing of rows or offs is written).  Every thread of the workgroup calls this.
__device__ __forceinline__ u64 take_hop(const ContSmallArgs& a, const MerkleT& t, const ContTakeHop& tk,
                                        const BucketPairs& bp, u64 j, u64 je, u32 c, u32 ko, u32 tot,
                                        const u64* s_pk, const u64* s_ph, u64* s_src, u32* s_wave) {
  const int tid = threadIdx.x;
  const u64 kept = min<u64>(tot, a.kcap);
  u64 rc = 0;  // the rows of this thread's kept keys
  u32 taken = 0;
  {
    u32 x = 0;
    auto emit = [&](u64 k, u64 r0, u64 n) __attribute__((always_inline)) {
      const u64 pos = (u64)ko + x++;
      if (pos < kept) {
        a.keys[pos] = k;
        rc += n;
      }
      if (n && !bp.big) taken |= 1u << (u32)(r0 - bp.r);
    };
    if (c) {
      if (bp.big)
        walk_global(a.s, t.th, bp.r, bp.re, s_pk, s_ph, j, je, emit);
      else
        walk_regs(bp, s_pk, s_ph, j, je, emit);
    }
  }
  // a bucket counts its rows in 32 bits: the sum of 512 of them, each clamped to 2^22, is exact
  // where it stays below 2^22; else the sums of the counts' 16-bit halves
  constexpr u32 SMALL = 1u << 22;
  u32 t32;
  u64 ro = block_excl_scan<CSN>((u32)min<u64>(rc, SMALL), s_wave, &t32), rtot = t32;
  if (t32 >= SMALL) {
    u32 tl, th2;
    const u32 el = block_excl_scan<CSN>((u32)(rc & 0xffffu), s_wave, &tl);
    const u32 eh = block_excl_scan<CSN>((u32)(rc >> 16), s_wave, &th2);
    ro = ((u64)eh << 16) + el;
    rtot = ((u64)th2 << 16) + tl;
  }
  if (rtot > tk.rcap) return rtot;
  if (tid == 0) tk.offs[kept] = rtot;
  for (u64 base = 0; base == 0 || base < rtot; base += CS_IN) {
    if (base) __syncthreads();  // the copy of the rows before
    u32 x = 0;
    u64 rq = ro;
    auto emit = [&](u64, u64 r0, u64 n) __attribute__((always_inline)) {
      const u64 pos = (u64)ko + x++;
      if (pos >= kept) return;
      if (base == 0) tk.offs[pos] = rq;
      const u64 lo = max(rq, base), hi = min(rq + n, base + (u64)CS_IN);
      for (u64 q = lo; q < hi; q++) s_src[q - base] = r0 + (q - rq);
      rq += n;
    };
    if (c) {
      if (bp.big)
        walk_global(a.s, t.th, bp.r, bp.re, s_pk, s_ph, j, je, emit);
      else
        walk_taken(bp, taken, s_pk, j, je, emit);
    }
    __syncthreads();
    const u64 m = min<u64>(rtot - base, (u64)CS_IN);
    for (u64 q = tid; q < m; q += CSN) {
      const u64 r = s_src[q];
      tk.rows.key[base + q] = a.s.key[r];
      tk.rows.val[base + q] = a.s.val[r];
      tk.rows.ts[base + q] = a.s.ts[r];
      tk.rows.node[base + q] = a.s.node[r];
      tk.rows.cnt[base + q] = a.s.cnt[r];
    }
  }
  return rtot;
}

template <bool BATCH, bool TAKE = false>
__global__ __launch_bounds__(CSN) void cont_hop_kernel(
    typename std::conditional<TAKE, ContTakeArgs,
                              typename std::conditional<BATCH, ContBatchArgs, ContSmallArgs>::type>::type p,
    MerkleT t) {
  static_assert(BATCH || !TAKE, "the take form is a batch hop");
  __shared__ u64 s_dpos[CS_IN];
  __shared__ u64 s_pk[CS_IN], s_ph[CS_IN];  // leaf form in: the peer's pairs; node form: bucket rows
  __shared__ u32 s_wave[CSN / WAVE + 1];
  __shared__ u32 s_bad;
  const ContSmallArgs& a = hop_args(p);
  const int tid = threadIdx.x;
  const u32 depth = t.depth, L = a.level;
  u64 h[CS_HDR] = {0, 0, 0, 0, 0, 0};  // the result header (every thread's copy is the same)
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (L <= depth) {
    // ---- node form: entries tid*PER .. +PER (consecutive: compaction keeps input order)
    u64 pos[CS_PER];
    u32 d = 0;
    const u64 lim = 1ull << L;
#pragma unroll
    for (u32 q = 0; q < CS_PER; q++) {
      const u64 i = (u64)tid * CS_PER + q;
      const bool ok = i < a.n;
      const u64 ic = ok ? i : 0;  // (n >= 1: the host handles an empty continuation)
      pos[q] = a.ipos[ic];
      const u64 hv = a.ihash[ic];
      if (ok && pos[q] >= lim) atomicOr(&s_bad, 1u);
      const u64 nv = t.nodes[(lim - 1) + (pos[q] < lim ? pos[q] : 0)];
      d |= (ok && pos[q] < lim && nv != hv) ? 1u << q : 0u;
    }
    u32 nd;
    const u32 o = block_excl_scan<CSN>((u32)__popc(d), s_wave, &nd);
    {
      u32 x = o;
#pragma unroll
      for (u32 q = 0; q < CS_PER; q++)
        if (d >> q & 1u) s_dpos[x++] = pos[q];
    }
    __syncthreads();
    if (s_bad) {
      h[0] = CS_BAD;
    } else if (nd == 0) {
      h[0] = CS_OK;  // {:ok, []}
    } else if (L < depth) {
      const u32 k = min(a.levels, depth - L);
      const u64 need = (u64)nd << k, m = min(need, a.max);
      h[3] = L + k;
      if (m > a.ocap) {
        h[0] = CS_CAP;
        h[4] = m;
      } else {
        const u64 mask = (1ull << k) - 1, base = (1ull << (L + k)) - 1;
        for (u64 j = tid; j < m; j += CSN) {
          const u64 p = (s_dpos[j >> k] << k) | (j & mask);
          a.opos[j] = p;
          a.ohash[j] = t.nodes[base + p];
        }
        h[0] = CS_NODE;
        h[1] = m;
      }
    } else {
      // the differing buckets -> leaf form, the first `max` of them: one bucket per thread,
      // its pairs made in registers (the generic loops past CSN buckets)
      const u64 nb = min<u64>(nd, a.max);
      h[3] = depth + 1;
      if (nb <= (u64)CSN) {
        BucketPairs bp;
        bp.big = false;
        bp.head = 0;
        bp.r = bp.re = 0;
        u64 b = 0;
        if ((u64)tid < nb) {
          b = s_dpos[tid];
          bucket_pairs(t, a.s, b, bp);
        }
        const u32 c = bp.big ? distinct_keys(a.s, bp.r, bp.re) : (u32)__popc(bp.head);
        u32 np;
        const u32 po = block_excl_scan<CSN>(c, s_wave, &np);
        if (np > a.ocap || nb > a.ocap_b) {
          h[0] = CS_CAP;
          h[4] = np;
          h[5] = nb;
        } else {
          if ((u64)tid < nb) {
            a.obucket[tid] = b;
            if (bp.big) {
              pairs_global(t, a.s, bp.r, bp.re, a.opos, a.ohash, po);
            } else {
              u64 o2 = po;
#pragma unroll
              for (int i = 0; i < BR; i++)
                if (bp.head >> i & 1u) {
                  a.opos[o2] = bp.key[i];
                  a.ohash[o2++] = bp.leaf[i];
                }
            }
          }
          h[0] = CS_LEAF;
          h[1] = np;
          h[2] = nb;
        }
      } else {
        u32 c = 0;  // this thread's buckets' distinct keys
        u64 r[CS_PER], re[CS_PER];
#pragma unroll
        for (u32 q = 0; q < CS_PER; q++) {
          const u64 u = (u64)tid * CS_PER + q;
          r[q] = re[q] = 0;
          if (u < nb) bucket_rows(t, a.s, s_dpos[u], r[q], re[q]);
          c += distinct_keys(a.s, r[q], re[q]);
        }
        u32 np;
        const u32 po = block_excl_scan<CSN>(c, s_wave, &np);
        if (np > a.ocap || nb > a.ocap_b) {
          h[0] = CS_CAP;
          h[4] = np;
          h[5] = nb;
        } else {
          u64 o2 = po;
#pragma unroll
          for (u32 q = 0; q < CS_PER; q++) {
            const u64 u = (u64)tid * CS_PER + q;
            if (u < nb) a.obucket[u] = s_dpos[u];
            o2 += pairs_global(t, a.s, r[q], re[q], a.opos, a.ohash, o2);
          }
          h[0] = CS_LEAF;
          h[1] = np;
          h[2] = nb;
        }
      }
    }
  } else {
    // ---- leaf form received (<= CS_B = CSN buckets): the peer's pairs staged, then one
    //      bucket per thread, its rows' (key, leaf) pairs in registers merged with them
    static_assert(CS_B <= (u32)CSN, "one bucket per thread");
    for (u64 i = tid; i < a.n; i += CSN) {
      s_pk[i] = a.ipos[i];
      s_ph[i] = a.ihash[i];
    }
    __syncthreads();
    BucketPairs bp;
    bp.big = false;
    bp.head = 0;
    bp.r = bp.re = 0;
    u64 j = 0, je = 0;
    u32 c = 0;
    if ((u64)tid < a.nb) {
      const u64 b = a.ibucket[tid];
      if (b >> depth) {
        atomicOr(&s_bad, 1u);
      } else {
        bucket_pairs(t, a.s, b, bp);
        j = bucket_start(t, s_pk, a.n, b);
        je = bucket_start(t, s_pk, a.n, b + 1);
        c = bp.big ? merge_big<false, TAKE>(a.s, t.th, bp.r, bp.re, s_pk, s_ph, j, je, nullptr, 0, 0)
                   : merge_regs<false>(bp, s_pk, s_ph, j, je, nullptr, 0, 0);
      }
    }
    u32 tot;
    const u32 ko = block_excl_scan<CSN>(c, s_wave, &tot);
    if (s_bad) {
      h[0] = CS_BAD;
    } else {
      bool plain = true;
      if constexpr (TAKE) {
        const ContTakeHop& tk = p.takes[blockIdx.x];
        if (tk.offs) {  // (uniform: the descriptor is the workgroup's)
          plain = false;
          const u64 rows = take_hop(a, t, tk, bp, j, je, c, ko, tot, s_pk, s_ph, s_dpos, s_wave);
          if (tid == 0) a.home[CS_TAKEN] = rows;  // (a word of the slot past the CS_HDR written below)
        }
      }
      if (plain && c) {
        if (bp.big)
          merge_big<true, TAKE>(a.s, t.th, bp.r, bp.re, s_pk, s_ph, j, je, a.keys, ko, a.kcap);
        else
          merge_regs<true>(bp, s_pk, s_ph, j, je, a.keys, ko, a.kcap);
      }
      h[0] = CS_OK;
      h[1] = tot;
    }
  }
  if (tid < CS_HDR) {
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < CS_HDR; i++) v = i == tid ? h[i] : v;
    a.home[tid] = v;
  }
  if constexpr (BATCH) {
    __threadfence_system();  // (1)
    __syncthreads();         // (2): also past every read of s_bad
    if (tid == 0) {
      const u32 arrived = __hip_atomic_fetch_add(p.arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = arrived == gridDim.x - 1;
      if (last) __hip_atomic_store(p.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_bad = last ? 1u : 0u;
    }
    __syncthreads();
    if (s_bad) {
      __threadfence_system();  // (3)
      publish_counts(p.d_counts, p.h_pub, p.seq);
    }
  } else {
    publish_counts(a.d_counts, a.h_pub, a.seq);
  }
}

}  // namespace

hipError_t launch_cont_prepare(const MerkleT& t, u32 L, u64* opos, u64* ohash, hipStream_t st) {
  hipLaunchKernelGGL(cont_prepare_kernel, dim3(grid_of(1ull << L, PB)), dim3(PB), 0, st, t, L, opos, ohash);
  return hipGetLastError();
}

hipError_t launch_cont_small(const ContSmallArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(cont_hop_kernel<false>, dim3(1), dim3(CSN), 0, st, a, a.t);
  return hipGetLastError();
}

hipError_t launch_cont_batch(const ContBatchArgs& p, u32 k, hipStream_t st) {
  hipLaunchKernelGGL(cont_hop_kernel<true>, dim3(k), dim3(CSN), 0, st, p, p.t);
  return hipGetLastError();
}

hipError_t launch_cont_take(const ContTakeArgs& p, u32 k, hipStream_t st) {
  hipLaunchKernelGGL((cont_hop_kernel<true, true>), dim3(k), dim3(CSN), 0, st, p, p.t);
  return hipGetLastError();
}

hipError_t launch_cont_compare(const MerkleT& t, u32 L, const u64* pos, const u64* hash, u64 n,
                               u64* scratch, u64* dpos, u64* d_count, hipStream_t st) {
  const u64 tiles = (n + PB - 1) / PB;
  if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  hipLaunchKernelGGL(cont_count_kernel, dim3((unsigned)tiles), dim3(PB), 0, st, t, L, pos, hash, n,
                     scratch);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(DSB), 0, st, scratch, scratch + tiles, tiles,
                     d_count);
  hipLaunchKernelGGL(cont_compact_kernel, dim3((unsigned)tiles), dim3(PB), 0, st, t, L, pos, hash, n,
                     scratch + tiles, dpos);
  return hipGetLastError();
}

hipError_t launch_cont_expand(const MerkleT& t, u32 L, u32 k, const u64* dpos, u64 nd, u64* opos,
                              u64* ohash, hipStream_t st) {
  if (nd == 0) return hipSuccess;
  hipLaunchKernelGGL(cont_expand_kernel, dim3(grid_of(nd << k, PB)), dim3(PB), 0, st, t, L, k,
                     dpos, nd, opos, ohash);
  return hipGetLastError();
}

hipError_t launch_leaves_count(const MerkleT& t, const Rows& s, const u64* buckets, u64 nb,
                               u64* scratch, u64* d_count, hipStream_t st) {
  const u64 tiles = (nb + PB - 1) / PB;
  if (nb == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  hipLaunchKernelGGL(leaves_kernel<false>, dim3((unsigned)tiles), dim3(PB), 0, st, t, s, buckets,
                     nb, scratch, (const u64*)nullptr, (u64*)nullptr, (u64*)nullptr);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(DSB), 0, st, scratch, scratch + tiles, tiles,
                     d_count);
  return hipGetLastError();
}

hipError_t launch_leaves_write(const MerkleT& t, const Rows& s, const u64* buckets, u64 nb,
                               const u64* scratch, u64* ok, u64* oh, hipStream_t st) {
  const u64 tiles = (nb + PB - 1) / PB;
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(leaves_kernel<true>, dim3((unsigned)tiles), dim3(PB), 0, st, t, s, buckets,
                     nb, (u64*)nullptr, scratch + tiles, ok, oh);
  return hipGetLastError();
}

hipError_t launch_leafdiff(const MerkleT& t, const Rows& s, const u64* buckets, u64 nb, const u64* pk,
                           const u64* ph, u64 np, u64* out, u64 cap, u64* scratch, u64* d_count,
                           hipStream_t st) {
  const u64 tiles = (nb + PB - 1) / PB;
  if (nb == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  hipLaunchKernelGGL(leafdiff_kernel<false>, dim3((unsigned)tiles), dim3(PB), 0, st, t, s, buckets, nb,
                     pk, ph, np, scratch, (const u64*)nullptr, (u64*)nullptr, (u64)0);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(DSB), 0, st, scratch, scratch + tiles, tiles,
                     d_count);
  hipLaunchKernelGGL(leafdiff_kernel<true>, dim3((unsigned)tiles), dim3(PB), 0, st, t, s, buckets, nb,
                     pk, ph, np, (u64*)nullptr, scratch + tiles, out, cap);
  return hipGetLastError();
}

hipError_t launch_pairs_before_bucket(const MerkleT& t, const u64* keys, u64 n, const u64* bucket,
                                     u64* d_count, hipStream_t st) {
  hipLaunchKernelGGL(pairs_before_kernel, dim3(1), dim3(64), 0, st, t, keys, n, bucket, d_count);
  return hipGetLastError();
}

}  // namespace dg
