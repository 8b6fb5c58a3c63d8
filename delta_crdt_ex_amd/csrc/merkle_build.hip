// merkle_build.hip — building and updating the Merkle tree (dg_tree.h describes it): the
// MerkleMap.put/delete per changed key and update_hashes of DeltaCrdt.CausalCrdt sync
// (reference lib/delta_crdt/causal_crdt.ex:390-394, :94,254).  merkle_map 0.2.0 is not
// vendored, so its hash and wire format are "parity unpinned" (SURVEY.md §8(c)); the role
// is reproduced exactly: a key's leaf depends on its raw value map (every {v, ts} entry and
// dot, :392), and two trees differ exactly above the keys whose raw value maps differ.
// The whole-tree diff is merkle_diff.hip, the partial diff merkle_cont.hip.
//
// Kernels (they share the chunk upsweep and the hand-off to the last workgroup):
//  * build: ONE launch.  A workgroup per chunk of 2^11 buckets streams the chunk's rows
//    (36 B/row; the row range from two wave lower bounds) into LDS bucket sums, reduces
//    the chunk's 11 levels in LDS and writes them; the last workgroup to finish (one
//    arrival counter, write-through hand-off words) reduces the chunk roots to the root.
//  * update: one thread per changed key re-hashes the key's rows in the old and the
//    new store and adds the difference to its bucket (put/delete); the upsweep then
//    re-reduces only the 2^11-bucket chunks an update touched (update_hashes).
//    kd_tree_kernel is the same put/delete from the count kernels' per-key figures (kdelta.hip,
//    kkeyed.hip; tree_put, dg_kdcount.h).
//  * kd_finish_kernel: the write of dg_join_delta's one-wait path (dg_kdw.h) and the dirty
//    chunks' re-reduction by persistent workgroups, in one launch.
#include "dg_kdw.h"
#include "dg_launch.h"
#include "dg_tree.h"

namespace dg {

namespace {

// ---------------------------------------------------------------- build / upsweep
// One workgroup per chunk of 2^L1 buckets (L1 = min(UPL, depth)).  BUILD: the chunk's
// rows (a contiguous range: two wave lower bounds) are hashed into LDS bucket sums
// (LDS atomic adds; no global atomics), UPDATE: the chunk's bucket level is read back
// (merkle_update_kernel has added the changed keys' deltas) -- only where the chunk is
// dirty.  Then L1 levels are reduced in LDS and written.  The last workgroup to finish
// reduces the chunk roots to the root and, for BUILD, sums the per-chunk distinct-key
// counts.  Hand-off (MI355X_MICROARCH.md "Valid forms", hand-off table row 1): ONE lane
// per workgroup stores the chunk's root and key count write-through (sc1), waits for
// them, then adds to ONE arrival counter; the workgroup whose add returns last reads the
// roots and counts with sc1 loads.  No release fence per workgroup: an agent release
// in each of 2048 workgroups cost 75 us of a 219 us build (rocprofv3 A/B).
#ifndef DG_MERKLE_VEC  // the build's 4-consecutive-rows loop (0: the strided loop, for A/B)
#define DG_MERKLE_VEC 1
#endif
constexpr bool MERKLE_VEC = DG_MERKLE_VEC;
constexpr int UPB = 512;   // threads per chunk workgroup
constexpr int UPL = MERKLE_UPL;  // levels reduced per workgroup (2048 nodes in LDS)
constexpr u32 UPW = 1u << UPL;
constexpr u32 NHL = 1024;  // node hashes staged in LDS by the build (more: read from global)

// s[0, width) holds level `hi` nodes g0 .. g0+width-1; reduce log2(width) levels in LDS
// and write every produced level (s ends with the subtree root in s[0]).
__device__ void lds_upsweep(u64* nodes, u32 hi, u64 g0, u32 width, u64* s) {
  u32 l = 0;
  for (u32 cnt = width >> 1; cnt >= 1; cnt >>= 1) {
    l++;
    u64* dst = nodes + ((1ull << (hi - l)) - 1) + (g0 >> l);
    u64 v[UPW / UPB / 2];
    int nv = 0;
    for (u32 x = threadIdx.x; x < cnt; x += UPB) v[nv++] = node_hash(s[2 * x], s[2 * x + 1]);
    __syncthreads();
    nv = 0;
    for (u32 x = threadIdx.x; x < cnt; x += UPB) {
      s[x] = v[nv];
      dst[x] = v[nv++];
    }
    __syncthreads();
  }
}

// The same for a full chunk (width == UPW == 4 * UPB) with ONE block barrier instead of
// eleven: a thread takes its 4 leaves from LDS and makes levels 1 and 2 in registers, each
// wave makes the next 6 levels with shuffles (at level 2 + k the lanes that are multiples
// of 2^k combine their node with the one 2^(k-1) lanes up), the 8 wave roots meet in LDS
// and wave 0 makes the last 3 levels.  Writes every level to `nodes` as lds_upsweep does
// and leaves the chunk root in s[0].
static_assert(UPW == 4 * UPB && UPB / WAVE == 8, "4 leaves per thread, 8 waves");
__device__ void chunk_upsweep(u64* nodes, u32 hi, u64 g0, u64* s) {
  const u32 tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  auto row = [&](u32 l) { return nodes + ((1ull << (hi - l)) - 1) + (g0 >> l); };
  const u64 l0 = s[4 * tid], l1 = s[4 * tid + 1], l2 = s[4 * tid + 2], l3 = s[4 * tid + 3];
  const u64 p0 = node_hash(l0, l1), p1 = node_hash(l2, l3);
  row(1)[2 * tid] = p0;
  row(1)[2 * tid + 1] = p1;
  u64 v = node_hash(p0, p1);
  row(2)[tid] = v;
#pragma unroll
  for (u32 k = 1; k <= 6; k++) {  // levels 3..8 inside the wave
    const u64 o = __shfl_down(v, 1u << (k - 1), WAVE);
    if ((lane & ((1u << k) - 1)) == 0) {
      v = node_hash(v, o);
      row(2 + k)[tid >> k] = v;
    }
  }
  __syncthreads();  // every wave is done reading s (the leaves)
  if (lane == 0) s[w] = v;  // level-8 node w
  __syncthreads();
  if (w == 0) {
    u64 x = lane < 8 ? s[lane] : 0ull;
#pragma unroll
    for (u32 k = 1; k <= 3; k++) {  // levels 9..11
      const u64 o = __shfl_down(x, 1u << (k - 1), WAVE);
      if (lane < 8 && (lane & ((1u << k) - 1)) == 0) {
        x = node_hash(x, o);
        row(8 + k)[lane >> k] = x;
      }
    }
    if (lane == 0) s[0] = x;
  }
  __syncthreads();
}

// The last workgroup of a chunk launch: levels depth - L1 .. 0, UPL levels per round (the
// first round's inputs are the handed-off chunk roots, sc1 loads), the chunk index moved
// by the chunks' row-count changes (cdelta, when given), and for a build the distinct-key
// count.  s: the caller's UPW-node LDS stage.
template <bool BUILD>
__device__ __forceinline__ void chunk_tail(MerkleT t, u64* hand, u64* d_keys, const i64* cdelta, const u64 G, u64* s) {
  const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  u32 hl = t.depth - L1;
  bool first = true;
  while (hl > 0) {
    const u32 nlev = hl < (u32)UPL ? hl : (u32)UPL;
    const u64 chunks = 1ull << (hl - nlev);
    const u64* src = t.nodes + ((1ull << hl) - 1);
    wait_vmem();  // this workgroup's own stores of level hl (depth > 2 * UPL) are complete
    __syncthreads();
    for (u64 c = 0; c < chunks; c++) {
      for (u32 x = tid; x < (1u << nlev); x += UPB)
        s[x] = first ? ld_sc1(hand + (c << nlev) + x) : src[(c << nlev) + x];
      __syncthreads();
      if ((1u << nlev) == UPW)  // (uniform)
        chunk_upsweep(t.nodes, hl, c << nlev, s);
      else
        lds_upsweep(t.nodes, hl, c << nlev, 1u << nlev, s);
    }
    hl -= nlev;
    first = false;
  }
  if (!BUILD && t.starts && cdelta) {
    // the update moved rows: chunk g's first row shifts by the row-count changes of the
    // chunks before it (an exclusive scan of cdelta, UPB chunks per round; the end by all)
    // (CP consecutive entries per thread, their loads issued together: one round of
    // UPB * CP = 4096 entries covers the 2048 chunks of a depth-22 tree)
    constexpr int CP = 4;
    i64 carry = 0;
    for (u64 c0 = 0; c0 <= G; c0 += (u64)UPB * CP) {
      const u64 x0 = c0 + (u64)tid * CP;
      i64 v[CP], st0[CP];
#pragma unroll
      for (int q = 0; q < CP; q++) {
        const u64 x = x0 + q;
        v[q] = x < G ? cdelta[x] : 0;
        st0[q] = x <= G ? (i64)t.starts[x] : 0;
      }
#pragma unroll
      for (int q = 0; q < CP; q++)  // consumed: zero again for the next update
        if (x0 + q < G && v[q]) ((i64*)cdelta)[x0 + q] = 0;
      i64 own = 0;
#pragma unroll
      for (int q = 0; q < CP; q++) own += v[q];
      i64 incl = own;
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        const i64 y = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += y;
      }
      __syncthreads();
      if (lane == WAVE - 1) s[w] = (u64)incl;
      __syncthreads();
      i64 before = 0, tot = 0;
      for (int q = 0; q < UPB / WAVE; q++) {
        const i64 y = (i64)s[q];
        before += q < w ? y : 0;
        tot += y;
      }
      i64 run = carry + before + incl - own;  // the changes of the chunks before x0
#pragma unroll
      for (int q = 0; q < CP; q++) {
        const u64 x = x0 + q;
        if (x <= G) t.starts[x] = (u64)(st0[q] + run);
        run += v[q];
      }
      carry += tot;
    }
  }
  if (BUILD) {
    u64 sum = 0;
    for (u64 x = tid; x < G; x += UPB) sum += ld_sc1(hand + G + x);
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, WAVE);
    __syncthreads();
    if (lane == 0) s[w] = sum;
    __syncthreads();
    if (tid == 0) {
      u64 tot = 0;
      for (int q = 0; q < UPB / WAVE; q++) tot += s[q];
      *d_keys = tot;
    }
  }
}

// ctr: the arrival counter, zero on entry and left zero (the last workgroup resets it: a
// persistent engine word, no fill launch per build); scratch: per chunk its root and its
// distinct-key count (u64 each, at hand[0, G) and hand[G, 2G)).
// (the body of one workgroup g of G)
template <bool BUILD, bool VEC = false>
__device__ __forceinline__ void chunk_block(Rows rows, MerkleT t, const u32* dirty, u32* ctr, u64* hand,
                                            u64* d_keys, u32* err, const i64* cdelta, const u64 g,
                                            const u64 G) {
  __shared__ u64 s[UPW];
  __shared__ u32 s_c[BUILD ? UPW : 1];  // rows per bucket
  __shared__ u64 s_nh[BUILD ? NHL : 1]; // node term hashes
  __shared__ u64 s_rng[2];
  __shared__ u32 s_red[UPB / WAVE];
  __shared__ u32 s_last;
  const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
  const u32 width = 1u << L1;
  const u64 g0 = g << L1;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  u64* lvl = t.nodes + ((1ull << t.depth) - 1);
  u64 chunk_root = 0, chunk_keys = 0;
  if (BUILD) {
    for (u32 x = tid; x < width; x += UPB) {
      s[x] = 0;
      s_c[x] = 0;
    }
    const bool nh_lds = t.th.on && t.th.nn <= NHL;  // uniform
    if (nh_lds)
      for (u32 x = tid; x < (u32)t.th.nn; x += UPB) s_nh[x] = t.th.nh[x];
    if (w < 2) {
      const u64 r = wave_bucket_start(t, rows.key, rows.n, g0 + (w ? width : 0));
      if (lane == 0) s_rng[w] = r;
    }
    __syncthreads();
    const u64 lo = s_rng[0], hi = s_rng[1];
    if (t.starts && tid == 0) {  // the chunk index (dg_merkle.starts): its first row, and the end
      t.starts[g] = lo;
      if (g == G - 1) t.starts[G] = hi;
    }
    u32 heads = 0;
    // rows outside the tree's key range (before the first chunk, after the last one)
    bool bad = tid == 0 && ((g == 0 && lo > 0) || (g == G - 1 && hi < rows.n));
    if (VEC) {
      // each thread hashes 4 CONSECUTIVE rows (16-byte loads: 2 per 8-byte column, 1 for
      // the node column), sums the rows of one bucket in registers and adds each run once
      // to LDS: ~1.4 LDS atomics per 4 rows instead of 8, and no two lanes of a wave add to
      // one bucket in the same instruction unless a bucket straddles them
      const u64 a0 = lo & ~3ull;
      const int lane_ = tid & (WAVE - 1);
      for (u64 base = a0; base < hi; base += 4 * UPB) {  // block-uniform trip count
        const u64 gb = base + 4 * (u64)tid;
        const bool any = gb < hi;
        u64 key[4] = {0, 0, 0, 0}, val[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
        i64 ts[4] = {0, 0, 0, 0};
        u32 nd[4] = {0, 0, 0, 0};
        // the previous row's key for lane 0, loaded by every lane at a clamped index with the
        // rows' own loads (a load under lane 0's branch was waited for on its own: build
        // 0.497 -> 0.510-0.516 of peak, A/B)
        const u64 pkey = rows.key[gb > 0 && gb - 1 < rows.n ? gb - 1 : 0];
        if (any && gb + 3 < rows.n) {
          const ulonglong2 k0 = *(const ulonglong2*)(rows.key + gb), k1 = *(const ulonglong2*)(rows.key + gb + 2);
          const ulonglong2 v0 = *(const ulonglong2*)(rows.val + gb), v1 = *(const ulonglong2*)(rows.val + gb + 2);
          const longlong2 t0 = *(const longlong2*)(rows.ts + gb), t1 = *(const longlong2*)(rows.ts + gb + 2);
          const ulonglong2 c0 = *(const ulonglong2*)(rows.cnt + gb), c1 = *(const ulonglong2*)(rows.cnt + gb + 2);
          const uint4 n4 = *(const uint4*)(rows.node + gb);
          key[0] = k0.x, key[1] = k0.y, key[2] = k1.x, key[3] = k1.y;
          val[0] = v0.x, val[1] = v0.y, val[2] = v1.x, val[3] = v1.y;
          ts[0] = t0.x, ts[1] = t0.y, ts[2] = t1.x, ts[3] = t1.y;
          cnt[0] = c0.x, cnt[1] = c0.y, cnt[2] = c1.x, cnt[3] = c1.y;
          nd[0] = n4.x, nd[1] = n4.y, nd[2] = n4.z, nd[3] = n4.w;
        } else if (any) {  // the store's last rows: no 16-byte load past its end
#pragma unroll
          for (int q = 0; q < 4; q++)
            if (gb + q < rows.n) {
              key[q] = rows.key[gb + q];
              val[q] = rows.val[gb + q];
              ts[q] = rows.ts[gb + q];
              cnt[q] = rows.cnt[gb + q];
              nd[q] = rows.node[gb + q];
            }
        }
        // the row before this thread's first: the previous lane's last key (lane 0: memory)
        u64 prev = __shfl_up(key[3], 1, WAVE);
        if (lane_ == 0) prev = (any && gb > 0) ? pkey : ~key[0];
        u64 run_h = 0;
        u32 run_c = 0;
        u64 run_b = ~0ull;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const u64 i = gb + (u64)q;
          if (i >= lo && i < hi) {
            const u64 nt = nh_lds ? (nd[q] < (u32)t.th.nn ? s_nh[nd[q]] : (u64)nd[q]) : th_node(t.th, nd[q]);
            const u64 h = row_hash(key[q], th_val(t.th, val[q]), ts[q], nt, cnt[q]);
            const u64 pk = q ? key[q - 1] : prev;
            heads += (i == lo || pk != key[q]) ? 1u : 0u;
            if (t.sb && (key[q] >> (64 - t.sb)) != t.shard) bad = true;
            const u64 b = bucket_of(t, key[q]) - g0;
            if (b != run_b) {
              if (run_b < width) {
                atomicAdd((unsigned long long*)&s[run_b], (unsigned long long)run_h);
                atomicAdd(&s_c[run_b], run_c);
              }
              run_b = b;
              run_h = 0;
              run_c = 0;
            }
            run_h += h;
            run_c++;
          }
        }
        if (run_b < width) {
          atomicAdd((unsigned long long*)&s[run_b], (unsigned long long)run_h);
          atomicAdd(&s_c[run_b], run_c);
        }
      }
    } else {
      for (u64 i0 = lo; i0 < hi; i0 += 4 * UPB) {
        u64 key[4], h[4];
        bool head[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {  // four rows in flight per thread
          const u64 i = i0 + (u64)q * UPB + tid;
          key[q] = 0;
          h[q] = 0;
          head[q] = false;
          if (i < hi) {
            key[q] = rows.key[i];
            const u32 nd = rows.node[i];
            const u64 nt = nh_lds ? (nd < (u32)t.th.nn ? s_nh[nd] : (u64)nd) : th_node(t.th, nd);
            h[q] = row_hash(key[q], th_val(t.th, rows.val[i]), rows.ts[i], nt, rows.cnt[i]);
            head[q] = i == lo || rows.key[i - 1] != key[q];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const u64 i = i0 + (u64)q * UPB + tid;
          if (i < hi) {
            if (t.sb && (key[q] >> (64 - t.sb)) != t.shard) bad = true;
            const u64 b = bucket_of(t, key[q]) - g0;
            if (b < width) {
              atomicAdd((unsigned long long*)&s[b], (unsigned long long)h[q]);
              atomicAdd(&s_c[b], 1u);
            }
            heads += head[q] ? 1u : 0u;
          }
        }
      }
    }
    // distinct keys of the chunk (keys of different chunks differ: a key fixes its bucket)
    u32 c = heads;
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) c += __shfl_xor(c, d, WAVE);
    if (lane == 0) s_red[w] = c;
    if (__ballot(bad) && lane == 0) atomicOr(err, ERR_SHARD);
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < UPB / WAVE; q++) chunk_keys += s_red[q];
    bool over = false;
    for (u32 x = tid; x < width; x += UPB) {
      lvl[g0 + x] = s[x];
      const u32 c = s_c[x];
      over |= c > 0xFFFFu;
      t.counts[g0 + x] = (uint16_t)(c > 0xFFFFu ? 0xFFFFu : c);
    }
    if (__ballot(over) && lane == 0) atomicOr(err, ERR_COUNT);
    if (width == UPW)  // (uniform)
      chunk_upsweep(t.nodes, t.depth, g0, s);
    else
      lds_upsweep(t.nodes, t.depth, g0, width, s);
    chunk_root = s[0];
  } else if (dirty && dirty[g]) {
    for (u32 x = tid; x < width; x += UPB) s[x] = lvl[g0 + x];
    __syncthreads();
    if (width == UPW)  // (uniform)
      chunk_upsweep(t.nodes, t.depth, g0, s);
    else
      lds_upsweep(t.nodes, t.depth, g0, width, s);
    chunk_root = s[0];
    if (tid == 0) ((u32*)dirty)[g] = 0;  // consumed: the flags are zero again for the next update
  } else if (tid == 0) {  // unchanged: its root as the previous kernels left it
    chunk_root = t.nodes[((1ull << (t.depth - L1)) - 1) + g];
  }
  // ---- hand the chunk root (and key count) to the last workgroup
  if (tid == 0) {
    st_sc1(hand + g, chunk_root);
    if (BUILD) st_sc1(hand + G + g, chunk_keys);
    wait_vmem();
    s_last = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1;
    if (s_last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all G arrived
  }
  __syncthreads();
  if (!s_last) return;
  chunk_tail<BUILD>(t, hand, d_keys, cdelta, G, s);
}

template <bool BUILD, bool VEC = false>
__global__ __launch_bounds__(UPB, 4) void merkle_chunk_kernel(Rows rows, MerkleT t, const u32* dirty,
                                                           u32* ctr, u64* hand, u64* d_keys,
                                                           u32* err, const i64* cdelta) {
  chunk_block<BUILD, VEC>(rows, t, dirty, ctr, hand, d_keys, err, cdelta, blockIdx.x, gridDim.x);
}

// The update's re-reduction by NB persistent workgroups, chunks g = cb, cb + NB, ...: a
// workgroup per chunk paid a dirty-flag load, a root load, a write-through hand-off and an
// arrival for every chunk, and 2048 such workgroups took 32 us with nothing dirty (A/B).
// Here a workgroup loads its chunks' flags and old roots in one round trip, re-reduces its
// dirty chunks one after the other (the next chunk's leaves issued before the current
// one's upsweep), hands every root off write-through and arrives once; the last one runs
// chunk_tail.  The leaves are double-buffered in LDS.
constexpr u32 KCH = 16;  // chunks per workgroup at most (G <= KCH * NB)
__device__ __forceinline__ void kd_chunks(MerkleT t, u32* dirty, u32* ctr, u64* hand, const i64* cdelta, const u64 cb,
                                          const u64 NB, const u64 G) {
  __shared__ u64 s2[2][UPW];
  __shared__ u32 s_fl[KCH];
  __shared__ u64 s_rt[KCH];
  __shared__ u32 s_last;
  const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
  const u32 width = 1u << L1;
  const int tid = threadIdx.x;
  const u64* lvl = t.nodes + ((1ull << t.depth) - 1);
  const u32 nc = (u32)((G - cb + NB - 1) / NB);  // this workgroup's chunks (<= KCH)
  if ((u32)tid < nc) {
    const u64 g = cb + (u64)tid * NB;
    s_fl[tid] = dirty[g];
    s_rt[tid] = t.nodes[((1ull << (t.depth - L1)) - 1) + g];
  }
  __syncthreads();
  // leaves of the i-th dirty chunk from position j on, into buffer b (registers first)
  auto next_dirty = [&](u32 j) {
    while (j < nc && !s_fl[j]) j++;
    return j;
  };
  u32 j = next_dirty(0);
  u64 v[UPW / UPB];
  if (j < nc)
#pragma unroll
    for (u32 q = 0; q < UPW / UPB; q++) {
      const u32 x = tid + q * UPB;
      v[q] = x < width ? lvl[((cb + (u64)j * NB) << L1) + x] : 0ull;
    }
  int b = 0;
  for (u32 i = 0; i < nc; i++) {
    const u64 g = cb + (u64)i * NB;
    if (i != j) {  // clean: its root as the previous kernels left it
      if (tid == 0) st_sc1(hand + g, s_rt[i]);
      continue;
    }
#pragma unroll
    for (u32 q = 0; q < UPW / UPB; q++) s2[b][tid + q * UPB] = v[q];
    __syncthreads();
    j = next_dirty(i + 1);  // the next dirty chunk's leaves in flight during this upsweep
    if (j < nc)
#pragma unroll
      for (u32 q = 0; q < UPW / UPB; q++) {
        const u32 x = tid + q * UPB;
        v[q] = x < width ? lvl[((cb + (u64)j * NB) << L1) + x] : 0ull;
      }
    if (width == UPW)  // (uniform)
      chunk_upsweep(t.nodes, t.depth, g << L1, s2[b]);
    else
      lds_upsweep(t.nodes, t.depth, g << L1, width, s2[b]);
    if (tid == 0) {
      st_sc1(hand + g, s2[b][0]);
      dirty[g] = 0;  // consumed: the flags are zero again for the next update
    }
    b ^= 1;
  }
  if (tid == 0) {
    wait_vmem();
    s_last = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == NB - 1;
    if (s_last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all NB arrived
  }
  __syncthreads();
  if (!s_last) return;
  chunk_tail<false>(t, hand, nullptr, cdelta, G, s2[0]);
}

// dg_join_delta's write (dg_kdw.h, workgroups [0, nw): dispatched first, they start at once)
// and the dirty chunks' re-reduction (the rest: kd_chunks' persistent workgroups) in ONE
// launch: both read only what kd_count_kernel wrote, so the write's ~15 us run under the
// re-reduction's instead of after it.
#ifndef DG_KDF_WAVES  // waves per SIMD the launch is compiled for: 6 = 73 VGPRs, three
#define DG_KDF_WAVES 6  // workgroups per CU, no spills (8 spills, 4 is two per CU: A/B slower)
#endif
__global__ __launch_bounds__(UPB, DG_KDF_WAVES) void kd_finish_kernel(KdArgs p, u32 nw, MerkleT t, const u32* dirty,
                                                         u32* ctr, u64* hand, const i64* cdelta) {
  if (blockIdx.x < nw) {
    kd_write_block<UPB>(p, blockIdx.x);
    return;
  }
  // no key's row count changed (the count kernel's moved flag): every chunk's row-count
  // change is zero, and the last workgroup skips the chunk index's scan
  const i64* cd = p.d_counts[KC_MOVED] ? cdelta : nullptr;
  const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
  kd_chunks(t, (u32*)dirty, ctr, hand, cd, blockIdx.x - nw, gridDim.x - nw, 1ull << (t.depth - L1));
}

// ---------------------------------------------------------------- update
constexpr int UB = 256;


// Σ row_hash of key x's rows in s (0 if absent); *rows = their number.
__device__ __forceinline__ u64 key_leaf(const Rows& s, u64 x, const TermH& th, u32* rows) {
  u64 i = interp_lower_bound(s.key, 0, s.n, x);
  u64 h = 0;
  u32 r = 0;
  for (; i < s.n && s.key[i] == x; i++, r++) h += rh(s, i, th);
  *rows = r;
  return h;
}

__global__ __launch_bounds__(UB) void merkle_update_kernel(MerkleT t, Rows olds, Rows news, const u64* keys,
                                                           u64 n_keys, u32* dirty, u64* d_keys,
                                                           u32* err, i64* cdelta) {
  const u64 i = (u64)blockIdx.x * UB + threadIdx.x;
  int dk = 0;
  bool bad = false, over = false;
  if (i < n_keys) {
    const u64 x = keys[i];
    u32 ro, rn;
    const u64 ho = key_leaf(olds, x, t.th, &ro), hn = key_leaf(news, x, t.th, &rn);
    dk = (int)(rn > 0) - (int)(ro > 0);
    if (ho != hn || ro != rn) {
      if (t.sb && (x >> (64 - t.sb)) != t.shard) {
        bad = true;
      } else {
        const u64 b = bucket_of(t, x);
        u64* lvl = t.nodes + ((1ull << t.depth) - 1);
        atomicAdd((unsigned long long*)&lvl[b], (unsigned long long)(hn - ho));
        if (rn != ro) {  // the bucket's row count, in its aligned 32-bit word (counts stay
                         // in [0, 65535]: no carry or borrow into the neighbour's half)
          u32* wd = (u32*)t.counts + (b >> 1);
          const u32 sh = 16u * (u32)(b & 1);
          if (rn > ro) {
            const u32 old = atomicAdd(wd, (rn - ro) << sh);
            over = ((old >> sh) & 0xFFFFu) + (rn - ro) > 0xFFFFu;
          } else {
            atomicSub(wd, (ro - rn) << sh);
          }
        }
        const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
        dirty[b >> L1] = 1u;
        if (cdelta && rn != ro)  // the chunk's rows changed in number: later chunks' starts move
          atomicAdd((unsigned long long*)&cdelta[b >> L1], (unsigned long long)((i64)rn - (i64)ro));
      }
    }
  }
  int c = dk;
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) c += __shfl_xor(c, d, WAVE);
  // 8 count shards (one word takes ~88 same-address atomics per us): d_keys[0, 8)
  if ((threadIdx.x & (WAVE - 1)) == 0 && c)
    atomicAdd((unsigned long long*)&d_keys[(blockIdx.x * (UB / WAVE) + threadIdx.x / WAVE) & 7],
              (unsigned long long)(long long)c);
  if (__ballot(bad) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(err, ERR_SHARD);
  if (__ballot(over) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(err, ERR_COUNT);
}

// The same put/delete from the count kernels' per-key figures (tree_put, dg_kdcount.h): key u
// changed (kd_run_chg of its runs word, dg_launch.h) with leaf change dh[u] and row-count
// change ne - na; sign -1 undoes sign +1.  The distinct-key
// change is the count kernel's (d_counts[KC_DKEYS]).  The keys are ascending: segmented sums
// over the lanes (seg_incl, dg_tree.h) leave ONE atomic per bucket and per chunk.
__global__ __launch_bounds__(UB) void kd_tree_kernel(MerkleT t, const u64* keys, const u64* runs, const u64* dh,
                                                     u64 nk, const u64* guard, int sign, u32* dirty,
                                                     u32* err, i64* cdelta) {
  if (guard && *guard) return;  // (uniform) the per-key figures are incomplete: nothing to apply
  const u64 i = (u64)blockIdx.x * UB + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const u32 L1 = t.depth < (u32)UPL ? t.depth : (u32)UPL;
  bool bad = false, over = false;
  u64 b = ~0ull, d = 0;
  int dr = 0, act = 0;
  if (i < nk) {
    const u64 rn = runs[i];
    const int na = (int)kd_run_na(rn), ne = (int)kd_run_ne(rn);
    const u64 x = keys[i];
    b = bucket_of(t, x);
    if (kd_run_chg(rn)) {
      const u64 dd = sign > 0 ? dh[i] : (u64)0 - dh[i];
      const int r = sign > 0 ? ne - na : na - ne;
      if (dd != 0 || r != 0) {
        if (t.sb && (x >> (64 - t.sb)) != t.shard) {
          bad = true;  // (skipped both ways)
        } else {
          d = dd;
          dr = r;
          act = 1;
        }
      }
    }
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
    if (sr) {  // the bucket's row count in its aligned 32-bit word (as merkle_update_kernel)
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
    dirty[c] = 1u;
    if (cdelta && cr) atomicAdd((unsigned long long*)&cdelta[c], (unsigned long long)(i64)cr);
  }
  if (__ballot(bad) && lane == 0) atomicOr(err, ERR_SHARD);
  if (__ballot(over) && lane == 0) atomicOr(err, ERR_COUNT);
}

}  // namespace

hipError_t launch_merkle_build(const Rows& s, const MerkleT& t, u64* d_keys, u32* arrive, u64* hand,
                               u32* err, hipStream_t st) {
  const u64 G = merkle_chunks(t.depth);
  // 16-byte row loads need 16-byte aligned columns (a view into a packed buffer may not be)
  const bool vec = MERKLE_VEC && !(((uintptr_t)s.key | (uintptr_t)s.val | (uintptr_t)s.ts |
                                    (uintptr_t)s.node | (uintptr_t)s.cnt) & 15);
  if (vec)
    hipLaunchKernelGGL((merkle_chunk_kernel<true, true>), dim3((unsigned)G), dim3(UPB), 0, st, s, t,
                       (const u32*)nullptr, arrive, hand, d_keys, err, (const i64*)nullptr);
  else
    hipLaunchKernelGGL((merkle_chunk_kernel<true, false>), dim3((unsigned)G), dim3(UPB), 0, st, s, t,
                       (const u32*)nullptr, arrive, hand, d_keys, err, (const i64*)nullptr);
  return hipGetLastError();
}

hipError_t launch_merkle_update(const MerkleT& t, const Rows& olds, const Rows& news, const u64* keys,
                                u64 n_keys, u32* dirty, u64* d_keys, u32* arrive, u64* hand, i64* cdelta,
                                u32* err, hipStream_t st) {
  const u64 G = merkle_chunks(t.depth);
  i64* cd = t.starts ? cdelta : nullptr;
  if (n_keys)
    hipLaunchKernelGGL(merkle_update_kernel, dim3(grid_of(n_keys, UB)), dim3(UB), 0, st, t, olds, news,
                       keys, n_keys, dirty, d_keys, err, cd);
  hipLaunchKernelGGL(merkle_chunk_kernel<false>, dim3((unsigned)G), dim3(UPB), 0, st, news, t, dirty,
                     arrive, hand, (u64*)nullptr, err, (const i64*)cd);
  return hipGetLastError();
}

hipError_t launch_kd_tree(const MerkleT& t, const u64* keys, const u64* runs, const u64* dh, u64 nk,
                          const u64* guard, int sign, u32* dirty, u32* arrive, u64* hand, i64* cdelta,
                          u32* err, hipStream_t st) {
  const u64 G = merkle_chunks(t.depth);
  i64* cd = t.starts ? cdelta : nullptr;
  if (nk)
    hipLaunchKernelGGL(kd_tree_kernel, dim3(grid_of(nk, UB)), dim3(UB), 0, st, t, keys, runs, dh, nk, guard,
                       sign, dirty, err, cd);
  Rows none{};
  hipLaunchKernelGGL(merkle_chunk_kernel<false>, dim3((unsigned)G), dim3(UPB), 0, st, none, t, dirty, arrive,
                     hand, (u64*)nullptr, err, (const i64*)cd);
  return hipGetLastError();
}

hipError_t launch_kd_finish(const KdArgs& p0, const u32* dirty, u32* arrive, u64* hand, const i64* cdelta,
                            hipStream_t st) {
  KdArgs p = p0;
  p.ntiles = (p.nk + KD_BLOCK - 1) / KD_BLOCK;
  const u64 nw = (p.nk + UPB - 1) / UPB;
  const MerkleT t = p.has_tree ? p.t : MerkleT{};
  const u64 G0 = p.has_tree ? merkle_chunks(t.depth) : 0;
  // persistent chunk workgroups: at most 512 (three workgroups per CU beside the write's),
  // at least G / KCH
  const u64 G = G0 ? std::max<u64>(std::min<u64>(G0, 512), (G0 + KCH - 1) / KCH) : 0;
  if (nw + G == 0) return hipSuccess;
  hipLaunchKernelGGL(kd_finish_kernel, dim3((unsigned)(nw + G)), dim3(UPB), 0, st, p, (u32)nw, t, dirty, arrive,
                     hand, t.starts ? cdelta : (const i64*)nullptr);
  return hipGetLastError();
}

}  // namespace dg
