// replay.hip — the key half of dg_replace_keysets: k journal records (storage.py: the changed
// keys of one applied delta and those keys' rows after it) become ONE edit of the state.  Record
// j names the keys keys_cat[key_off[j], key_off[j + 1]) and holds their rows in the segment
// rows[row_off[j], row_off[j + 1]); for every key the LAST record naming it decides, and a
// record naming a key without rows removes it.  What the kernels here leave is what the splice
// (splice.hip) takes: the union of the keys, ascending, and per union key where the winning
// record's rows of it lie -- take.hip's copy then writes the edit store in key order from those
// (lo, len) pairs, exactly as it copies a located keyset out of a state.
//
//  1. replay_check_kernel: one thread per item (a key of a record) and per row.  The item finds
//     its record by a search of key_off (record numbers are positions, not mask bits: k is not
//     capped), compares itself with its predecessor in the keyset, and locates its key's run in
//     its own record's segment (a binary search of the segment, then a walk of the run: a key
//     has a few rows).  The run lengths are summed: a row whose key its record does not name is
//     in no run, so the sum then falls short of the row count.  The row compares itself with
//     its predecessor in its segment on the full tuple (store order).  Errors are bits of the
//     call's input-error word; nothing but scratch has been written when the host reads them.
//  2. sort_fields (sort.hip) orders the items by key.  The sort is stable and item positions
//     ascend with the record, so equal keys come out as one run in record order.
//  3. replay_union_kernel<false>, replay_scan_kernel, replay_union_kernel<true>: the tails of the
//     runs (an item whose successor holds another key) are the union, and a tail is its key's
//     winner.  Count per tile, one workgroup scans the tile counts, the write pass places key,
//     lo and len of every tail.  Three launches: no workgroup waits on another, so nothing here
//     depends on residency or dispatch order, and there is no spin to time out.
//
// No step depends on the key distribution: tiles are cut by item count.
//
// Budget (as compiled for gfx950).  replay_check_kernel: 256 threads, 8 B of LDS (the run sum),
// 17 VGPRs (the full-tuple compare loads its fields as it goes), so neither limits residency
// below 8 workgroups per CU; its loads are dependent searches, hidden by occupancy.
// replay_union_kernel: 256 threads x 4 items, LDS 8 B x (RP_TILE + 1) keys + the scan words =
// 8,232 B (19 workgroups' worth per CU: the 8-workgroup limit binds first), 12 VGPRs counting
// and 20 writing.  replay_scan_kernel: one workgroup, 32 B of LDS, 20 VGPRs.  No scratch.
#include "dg_launch.h"

namespace dg {

namespace {

constexpr int RB = RP_BLOCK, RI = RP_ITEMS, RT = RP_TILE;

// the last j in [0, k) with off[j] <= x (off ascending, off[0] <= x < off[k]: the host checked)
__device__ __forceinline__ u64 segment_of(const u64* off, u64 k, u64 x) {
  u64 a = 0, b = k;
  while (b - a > 1) {
    const u64 mid = (a + b) >> 1;
    if (off[mid] <= x)
      a = mid;
    else
      b = mid;
  }
  return a;
}

__global__ __launch_bounds__(RB) void replay_check_kernel(ReplayArgs p) {
  __shared__ unsigned long long s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const u64 t = (u64)blockIdx.x * RB + threadIdx.x;
  u32 bad = 0;
  if (t < p.m) {
    const u64 j = segment_of(p.key_off, p.k, t);
    const u64 key = p.keys_cat[t];
    if (t > p.key_off[j] && p.keys_cat[t - 1] >= key) bad |= RP_ERR_KEYS;
    const u64 r0 = p.row_off[j], r1 = p.row_off[j + 1];
    const u64 lo = lower_bound(p.rows.key, r0, r1, key);
    u64 e = lo;
    while (e < r1 && p.rows.key[e] == key) e++;
    p.item_lo[t] = lo;
    p.item_len[t] = (u32)(e - lo);  // (a run of 2^32 rows: the sum then differs from the row count)
    if (e > lo) atomicAdd(&s_sum, (unsigned long long)(e - lo));
  }
  if (t < p.rows.n) {
    const u64 j = segment_of(p.row_off, p.k, t);
    if (t > p.row_off[j] && row_cmp(load_row(p.rows, t - 1), load_row(p.rows, t)) >= 0) bad |= RP_ERR_ROWS;
  }
  if (bad) atomicOr(p.err, bad);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd((unsigned long long*)p.d_sum, s_sum);
}

// WRITE false: cnt[tile] = the tile's tails.  WRITE true: tail number off[tile] + (its rank in
// the tile) gets its key and the winning item's (lo, len).
template <bool WRITE>
__global__ __launch_bounds__(RB) void replay_union_kernel(const u64* cat, const u32* idx, u64 m, u64* cnt,
                                                          const u64* off, const u64* item_lo,
                                                          const u32* item_len, u64* ukeys, u64* u_lo,
                                                          u32* u_len) {
  __shared__ u64 s_key[RT + 1];  // s_key[i]: the tile's item i; s_key[nt]: the item behind the tile
  __shared__ u32 s_wave[RB / WAVE + 1];
  const u64 i0 = (u64)blockIdx.x * RT;
  const u32 nt = (u32)min<u64>(RT, m - i0);
#pragma unroll
  for (int q = 0; q < RI; q++) {
    const u32 li = q * RB + threadIdx.x;
    if (li < nt) s_key[li] = cat[idx ? idx[i0 + li] : i0 + li];
  }
  if (threadIdx.x == 0 && i0 + nt < m) s_key[nt] = cat[idx ? idx[i0 + nt] : i0 + nt];
  __syncthreads();
  const u32 l0 = threadIdx.x * RI;
  bool tail[RI];
  u32 c = 0;
#pragma unroll
  for (int q = 0; q < RI; q++) {
    const u32 li = l0 + q;
    tail[q] = li < nt && (i0 + li + 1 == m || s_key[li] != s_key[li + 1]);
    c += tail[q] ? 1u : 0u;
  }
  u32 total;
  const u32 excl = block_excl_scan<RB>(c, s_wave, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  u64 g = off[blockIdx.x] + excl;
#pragma unroll
  for (int q = 0; q < RI; q++) {
    if (!tail[q]) continue;
    const u32 li = l0 + q;
    const u64 w = idx ? idx[i0 + li] : i0 + li;  // the winner: the run's last item
    ukeys[g] = s_key[li];                        // (g < m: no more tails than items)
    u_lo[g] = item_lo[w];
    u_len[g] = item_len[w];
    g++;
  }
}

__global__ __launch_bounds__(RB) void replay_scan_kernel(const u64* cnt, u64* off, u64 ntiles, u64* d_count) {
  __shared__ u32 s_wave[RB / WAVE + 1];
  __shared__ u64 s_carry;
  scan_tile_counts<RB>(cnt, off, ntiles, d_count, s_wave, &s_carry);  // (a count is <= RP_TILE)
}

}  // namespace

hipError_t launch_replay_check(const ReplayArgs& p, hipStream_t st) {
  const u64 n = p.m > p.rows.n ? p.m : p.rows.n;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(replay_check_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(RB), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_replay_union(const u64* keys_cat, const u32* idx, u64 m, const u64* item_lo,
                               const u32* item_len, u64* tile_cnt, u64* tile_off, u64* ukeys, u64* u_lo,
                               u32* u_len, u64* d_count, hipStream_t st) {
  const u64 ntiles = replay_tiles(m);
  if (ntiles == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  hipLaunchKernelGGL(replay_union_kernel<false>, dim3((unsigned)ntiles), dim3(RB), 0, st, keys_cat, idx, m,
                     tile_cnt, tile_off, item_lo, item_len, ukeys, u_lo, u_len);
  hipLaunchKernelGGL(replay_scan_kernel, dim3(1), dim3(RB), 0, st, tile_cnt, tile_off, ntiles, d_count);
  hipLaunchKernelGGL(replay_union_kernel<true>, dim3((unsigned)ntiles), dim3(RB), 0, st, keys_cat, idx, m,
                     tile_cnt, tile_off, item_lo, item_len, ukeys, u_lo, u_len);
  return hipGetLastError();
}

}  // namespace dg
