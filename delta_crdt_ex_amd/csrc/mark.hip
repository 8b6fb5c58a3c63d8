// mark.hip — which ids of a host interning table do the resident stores still hold
// (dg_mark_ids)?
//
// The host's key and value tables only grow (interning.py Universe, c_src/marshal.c): a
// value that a later add replaced keeps its term, order key and hash for the life of the
// engine.  Only the device knows which ids its rows still name, and the val column is not
// sorted globally, so the question is one streaming pass over the chosen column of every
// store: 8 B read per row, a search of the (ascending) id table, and one bit set per id
// that occurs.  Three kernels on the engine stream, one host wait:
//
//   mark_prep_kernel    zeroes the bitmap and the call's counters
//   mark_kernel<MODE>   the pass: a grid-stride loop over tiles of the stores' concatenated rows
//                       (a small device table of column pointers, lengths and first tiles
//                       makes every store part of one launch), 16 B per lane and load.  A
//                       tile is 2048 rows; on the key column 512 while that gives at most
//                       4096 tiles (1M keys: 56 us against 86 us; a tile's window search is
//                       a chain of dependent loads, and 489 workgroups leave most CUs with
//                       one).  On the value column the smaller tiles measured slower (1M
//                       rows: 43 against 34 us at 2048 ids, 253 against 180 us at 100k).  A row whose id equals the one before it (the same
//                       thread's, or the previous lane's) is not searched: it takes that
//                       row's answer.  The searches by table size and column:
//                         MARK_STAGED   n_ids <= 2048: the table staged in LDS once per
//                                       workgroup (as remap.hip does)
//                         MARK_SAMPLED  the value column, larger tables: every stride-th id
//                                       (2048 samples at most, gathered once by the prep
//                                       kernel) staged in LDS, then a search of one stride of
//                                       the table in global memory (L2)
//                         MARK_WINDOW   the key column, larger tables: rows and table are
//                                       both sorted, so a tile's keys lie in one window of the
//                                       table, found by two wave-wide searches per tile; a
//                                       window of <= 2048 ids is staged in LDS, a larger one
//                                       searched in global memory
//                       Marks: where the table or the window is staged in LDS, so is its
//                       bitmap (test, then LDS atomicOr), flushed to the global bitmap once
//                       per workgroup or tile.  Otherwise a found id's bit is tested with an
//                       L2 load and set with a global atomicOr only while it reads clear (many
//                       rows share an id; an unconditional atomic per row would keep dropping
//                       the word's line from the L2).  A stale read of a set bit only costs
//                       a redundant atomicOr.
//   mark_finish_kernel  expands the bitmap into the caller's byte flags, counts them and
//                       verifies that the table is strictly ascending (a table that is not
//                       would make live ids look dead: the call reports DG_E_ORDER)
//
// MARK_WINDOW relies on the stores' own order (key ascending, the invariant of every store):
// a key outside its tile's first and last keys would be counted unknown, never marked.
#include "dg_launch.h"

namespace dg {

namespace {

constexpr int MB = 256;               // threads per workgroup
constexpr int MLDS = MARK_LDS_IDS;    // table entries staged in LDS (16 KB)
static_assert(MARK_TILE_SMALL == (u64)MB * 2 && MARK_TILE % MARK_TILE_SMALL == 0,
              "a tile is 1 or MARK_TILE / 512 row pairs per thread");
constexpr u64 NOT_FOUND = ~0ull;
constexpr u64 CANON_ID_LO = 1ull << 58, CANON_ID_HI = 1ull << 63;  // canonical integer values

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// index of x in t[lo, hi) (ascending), or NOT_FOUND
__device__ __forceinline__ u64 find_in(const u64* t, u64 lo, u64 hi, u64 x) {
  const u64 end = hi;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (t[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < end && t[lo] == x) ? lo : NOT_FOUND;
}

// The test reads through the L2 (an agent-scope load): a plain load is served by the CU's L1,
// which never sees another CU's atomicOr, so nearly every row found its bit "clear" and
// issued the atomic (measured: 1M rows over a 2048-id table took 150 us, most of it atomics
// queueing on two cache lines).
__device__ __forceinline__ void set_bit(u32* bitmap, u64 j) {
  u32* w = bitmap + (j >> 5);
  const u32 b = 1u << (j & 31);
  if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b)) atomicOr(w, b);
}

// The same in a workgroup's LDS bitmap (LDS reads are coherent within the workgroup).
__device__ __forceinline__ void set_bit_lds(u32* s_bm, u64 j) {
  u32* w = s_bm + (j >> 5);
  const u32 b = 1u << (j & 31);
  if (!(*w & b)) atomicOr(w, b);
}

constexpr int MBM = MLDS / 32 + 2;  // LDS bitmap words: 2048 ids from any bit of the first word

// the LDS bitmap's nonzero words into the global one, from word g0 on
__device__ __forceinline__ void flush_bits(const u32* s_bm, u32* bitmap, u64 g0) {
  for (int k = threadIdx.x; k < MBM; k += MB) {
    const u32 v = s_bm[k];
    if (v && (__hip_atomic_load(bitmap + g0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & v) != v)
      atomicOr(bitmap + g0 + k, v);
  }
}

struct Window {  // MARK_WINDOW: the tile's slice of the table
  u64 lo, hi;
  bool staged;
};

template <int MODE>
__device__ __forceinline__ u64 lookup(const u64* s_tab, const u64* ids, u64 n_ids, u64 stride,
                                      u64 n_samples, const Window& w, u64 x) {
  if (MODE == MARK_STAGED) return find_in(s_tab, 0, n_ids, x);
  if (MODE == MARK_SAMPLED) {
    // p: the first sample >= x; x, if present, is that sample or lies in the stride before it
    u64 lo = 0, hi = n_samples;
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (s_tab[mid] < x)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < n_samples && s_tab[lo] == x) return lo * stride;
    if (lo == 0) return NOT_FOUND;
    const u64 a = (lo - 1) * stride + 1;
    const u64 b = lo * stride < n_ids ? lo * stride : n_ids;
    return find_in(ids, a, b, x);
  }
  if (w.staged) {
    const u64 j = find_in(s_tab, 0, w.hi - w.lo, x);
    return j == NOT_FOUND ? j : w.lo + j;
  }
  return find_in(ids, w.lo, w.hi, x);
}

// (MARK_SAMPLED: also gathers the samples once, contiguous, so that a workgroup of the pass
// stages 16 KB instead of 2048 strided cache lines)
__global__ __launch_bounds__(MB) void mark_prep_kernel(u32* bitmap, u64 words, u64* d_counts, u32* bad,
                                                       const u64* ids, u64 stride, u64 n_samples, u64* samples) {
  for (u64 i = (u64)blockIdx.x * MB + threadIdx.x; i < words; i += (u64)gridDim.x * MB) bitmap[i] = 0;
  for (u64 i = (u64)blockIdx.x * MB + threadIdx.x; i < n_samples; i += (u64)gridDim.x * MB)
    samples[i] = ids[i * stride];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d_counts[0] = 0;
    d_counts[1] = 0;
    *bad = 0;
  }
}

template <int MODE, int COL>
__global__ __launch_bounds__(MB) void mark_kernel(const MarkSeg* segs, u64 n_segs, u64 n_tiles,
                                                  u32 iters, const u64* ids, u64 n_ids, u64 stride,
                                                  u64 n_samples, const u64* samples, u32* bitmap,
                                                  u64* d_unknown) {
  const u64 tile_rows = (u64)MB * 2 * iters;  // 16-byte loads per thread and tile: iters
  __shared__ u64 s_tab[MLDS];
  __shared__ u64 s_win[2];
  // marks of a table (MARK_STAGED) or a tile's window (MARK_WINDOW) that is staged in LDS are
  // collected in an LDS bitmap and flushed once: a few dozen global atomics per workgroup or
  // tile instead of up to one per row
  __shared__ u32 s_bm[MBM];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  if (MODE == MARK_STAGED) {
    for (u64 i = tid; i < n_ids; i += MB) s_tab[i] = ids[i];
    for (int k = tid; k < MBM; k += MB) s_bm[k] = 0;
    __syncthreads();
  } else if (MODE == MARK_SAMPLED) {
    for (u64 i = tid; i < n_samples; i += MB) s_tab[i] = samples[i];
    __syncthreads();
  }
  u32 unknown = 0;
  u64 seg = 0;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    while (seg + 1 < n_segs && segs[seg + 1].tile0 <= tile) seg++;  // (empty stores: no tiles)
    const u64* col = segs[seg].col;
    const u64 n = segs[seg].n;
    const u64 r0 = (tile - segs[seg].tile0) * tile_rows;
    const u64 r1 = r0 + tile_rows < n ? r0 + tile_rows : n;
    Window w{0, 0, false};
    if (MODE == MARK_WINDOW) {
      __syncthreads();  // the previous tile's searches of s_tab and reads of s_win are done
      if (wv == 0) {
        const u64 lo = wave_lower_bound(ids, n_ids, col[r0]);
        if (lane == 0) s_win[0] = lo;
      } else if (wv == 1) {
        const u64 k1 = col[r1 - 1];
        const u64 hi = k1 == ~0ull ? n_ids : wave_lower_bound(ids, n_ids, k1 + 1);
        if (lane == 0) s_win[1] = hi;
      }
      __syncthreads();
      w.lo = s_win[0];
      w.hi = s_win[1] > w.lo ? s_win[1] : w.lo;  // (an unsorted table: keep the window well-formed)
      w.staged = w.hi - w.lo <= (u64)MLDS;
      if (w.staged) {
        for (u64 i = tid; i < w.hi - w.lo; i += MB) s_tab[i] = ids[w.lo + i];
        for (int k = tid; k < MBM; k += MB) s_bm[k] = 0;
        __syncthreads();
      }
    }
    // where this tile's marks go: the LDS bitmap (bit j - bm_base) or the global one
    const bool lds_bits = MODE == MARK_STAGED || (MODE == MARK_WINDOW && w.staged);
    const u64 bm_base = MODE == MARK_WINDOW ? (w.lo & ~31ull) : 0;
    const bool vec = (((uintptr_t)col) & 15) == 0;
#pragma unroll 1
    for (u32 it = 0; it < iters; it++) {
      const u64 i = r0 + ((u64)it * MB + tid) * 2;
      const bool va = i < r1, vb = i + 1 < r1;
      u64 a = 0, b = 0;
      if (vb) {
        if (vec) {
          const u64x2 p = *(const u64x2*)(col + i);
          a = p.x;
          b = p.y;
        } else {
          a = col[i];
          b = col[i + 1];
        }
      } else if (va) {
        a = col[i];
      }
      // the previous lane's second id (lane 0 of a wave gets a value that differs from a).
      // The rows of one step ascend with the lane and the valid ones form a prefix, so a
      // valid row's previous lane holds two valid rows.
      const u32 pl = wave_prev_or((u32)b, ~(u32)a);
      const u32 ph = wave_prev_or((u32)(b >> 32), (u32)(a >> 32));
      const bool skip_a = va && (((u64)ph << 32) | pl) == a;
      const bool skip_b = vb && b == a;
      bool unk_a = false, unk_b = false;
      if (va && !skip_a && !(COL == DG_MARK_COL_VAL && a >= CANON_ID_LO && a < CANON_ID_HI)) {
        const u64 j = lookup<MODE>(s_tab, ids, n_ids, stride, n_samples, w, a);
        if (j == NOT_FOUND)
          unk_a = true;
        else if (lds_bits)
          set_bit_lds(s_bm, j - bm_base);
        else
          set_bit(bitmap, j);
      }
      if (vb && !skip_b && !(COL == DG_MARK_COL_VAL && b >= CANON_ID_LO && b < CANON_ID_HI)) {
        const u64 j = lookup<MODE>(s_tab, ids, n_ids, stride, n_samples, w, b);
        if (j == NOT_FOUND)
          unk_b = true;
        else if (lds_bits)
          set_bit_lds(s_bm, j - bm_base);
        else
          set_bit(bitmap, j);
      }
      // the answers of the rows that were not searched: a lane that searched either of its
      // rows knows its last row's answer itself (lane 0 always does); a lane whose first row
      // was skipped takes the answer of the nearest such lane below it
      const bool definite = !(skip_a && skip_b);
      const bool last = skip_b ? unk_a : unk_b;
      const u64 dmask = __ballot(definite), rmask = __ballot(definite && last);
      if (skip_a) {
        const u64 below = dmask & ((1ull << lane) - 1);
        const int src = 63 - __clzll((long long)below);
        unk_a = (rmask >> src) & 1;
      }
      if (skip_b) unk_b = unk_a;
      unknown += (va && unk_a ? 1u : 0u) + (vb && unk_b ? 1u : 0u);
    }
    if (MODE == MARK_WINDOW && w.staged) {
      __syncthreads();
      flush_bits(s_bm, bitmap, bm_base >> 5);
    }
  }
  if (MODE == MARK_STAGED) {
    __syncthreads();
    flush_bits(s_bm, bitmap, 0);
  }
  const u32 s = wave_sum_u32(unknown);
  if (lane == 0 && s) atomicAdd((unsigned long long*)d_unknown, (unsigned long long)s);
}

// used[j] = bit j of the bitmap, d_counts[0] += the ones, *bad |= 1 where ids[j] >= ids[j + 1]
__global__ __launch_bounds__(MB) void mark_finish_kernel(const u32* bitmap, const u64* ids, u64 n_ids,
                                                         uint8_t* used, u64* d_counts, u32* bad) {
  const uint8_t* bytes = (const uint8_t*)bitmap;
  const u64 groups = (n_ids + 7) / 8;
  const bool aligned = (((uintptr_t)used) & 7) == 0;
  const int lane = threadIdx.x & (WAVE - 1);
  u32 ones = 0;
  bool unordered = false;
  for (u64 g = (u64)blockIdx.x * MB + threadIdx.x; g < groups; g += (u64)gridDim.x * MB) {
    const u64 j0 = g * 8;
    const u32 m = n_ids - j0 >= 8 ? 8u : (u32)(n_ids - j0);
    const u32 bits = (u32)bytes[g] & ((1u << m) - 1u);
    ones += (u32)__popc(bits);
    if (m == 8 && aligned) {
      u64 v = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) v |= (u64)((bits >> k) & 1u) << (8 * k);
      *(u64*)(used + j0) = v;
    } else {
      for (u32 k = 0; k < m; k++) used[j0 + k] = (uint8_t)((bits >> k) & 1u);
    }
    u64 prev = ids[j0];
    for (u32 k = 1; k <= m; k++) {
      if (j0 + k >= n_ids) break;
      const u64 cur = ids[j0 + k];
      unordered |= prev >= cur;
      prev = cur;
    }
  }
  const u32 s = wave_sum_u32(ones);
  if (lane == 0 && s) atomicAdd((unsigned long long*)d_counts, (unsigned long long)s);
  if (unordered) atomicOr(bad, 1u);
}

template <int MODE>
void launch_mode(int column, unsigned grid, hipStream_t st, const MarkSeg* segs, u64 n_segs, u64 n_tiles,
                 u32 iters, const u64* ids, u64 n_ids, u64 stride, u64 n_samples, const u64* samples,
                 u32* bitmap, u64* d_unknown) {
  if (column == DG_MARK_COL_VAL)
    hipLaunchKernelGGL((mark_kernel<MODE, DG_MARK_COL_VAL>), dim3(grid), dim3(MB), 0, st, segs, n_segs,
                       n_tiles, iters, ids, n_ids, stride, n_samples, samples, bitmap, d_unknown);
  else
    hipLaunchKernelGGL((mark_kernel<MODE, DG_MARK_COL_KEY>), dim3(grid), dim3(MB), 0, st, segs, n_segs,
                       n_tiles, iters, ids, n_ids, stride, n_samples, samples, bitmap, d_unknown);
}

}  // namespace

int mark_mode(int column, u64 n_ids) {
  if (n_ids <= (u64)MLDS) return MARK_STAGED;
  return column == DG_MARK_COL_KEY ? MARK_WINDOW : MARK_SAMPLED;
}

hipError_t launch_mark_ids(const MarkSeg* segs, u64 n_segs, u64 n_tiles, u64 tile_rows, int column, int mode,
                           const u64* ids, u64 n_ids, u32* bitmap, u64* samples, uint8_t* used, u64* d_counts,
                           u32* bad, hipStream_t st) {
  const u64 words = mark_bitmap_words(n_ids);
  u64 pb = (words + MB - 1) / MB;
  pb = pb < 1 ? 1 : (pb > 1024 ? 1024 : pb);
  const u64 stride = (n_ids + MLDS - 1) / MLDS;  // MARK_SAMPLED: >= 2 there
  const u64 n_samples = mode == MARK_SAMPLED ? (n_ids + stride - 1) / stride : 0;
  hipLaunchKernelGGL(mark_prep_kernel, dim3((unsigned)pb), dim3(MB), 0, st, bitmap, words, d_counts, bad, ids,
                     stride, n_samples, samples);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  if (n_tiles) {
    const unsigned grid = (unsigned)(n_tiles < MARK_MAX_GRID ? n_tiles : MARK_MAX_GRID);
    const u32 iters = (u32)(tile_rows / MARK_TILE_SMALL);
    if (mode == MARK_STAGED)
      launch_mode<MARK_STAGED>(column, grid, st, segs, n_segs, n_tiles, iters, ids, n_ids, stride, n_samples,
                               samples, bitmap, d_counts + 1);
    else if (mode == MARK_SAMPLED)
      launch_mode<MARK_SAMPLED>(column, grid, st, segs, n_segs, n_tiles, iters, ids, n_ids, stride, n_samples,
                                samples, bitmap, d_counts + 1);
    else
      launch_mode<MARK_WINDOW>(column, grid, st, segs, n_segs, n_tiles, iters, ids, n_ids, stride, n_samples,
                               samples, bitmap, d_counts + 1);
    rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  if (n_ids) {
    u64 fb = ((n_ids + 7) / 8 + MB - 1) / MB;
    fb = fb > 1024 ? 1024 : fb;
    hipLaunchKernelGGL(mark_finish_kernel, dim3((unsigned)fb), dim3(MB), 0, st, bitmap, ids, n_ids, used,
                       d_counts, bad);
    rc = hipGetLastError();
  }
  return rc;
}

}  // namespace dg
