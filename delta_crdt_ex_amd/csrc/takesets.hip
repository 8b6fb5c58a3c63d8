// takesets.hip — the key half of dg_take_keysets: k ascending keysets (the keys of k pending
// {:get_diff, diff, keys} / send_diff messages, causal_crdt.ex:112-123 and :324-335) become
// their union, ascending and unique, with a u64 mask per union key (bit j: keyset j holds it).
// The rows are then taken ONCE for the union by take.hip, whose per-key offsets say which
// rows belong to which key and so, through the masks, to which message.
//
// Shape: (key, set) pairs through sort.hip's stable radix sort, then a run-detect pass.  (For a
// few thousand items dg_join_deltas_keyed gets the sorted pairs from keysets_rank_kernel instead.)
//
//  1. keysets_gather_kernel lays the keysets end to end: cat[p] = the key, set[p] = its
//     keyset (u8), and compares every key with its predecessor in its keyset in the same
//     pass (a keyset that is not strictly ascending sets the call's input-error word; the
//     host stops there, so the later kernels only ever see unique keysets).
//  2. sort_fields orders the items by key.  The sort is stable and the items lie in keyset
//     order, so equal keys come out as ONE run, ascending by keyset, of at most k <= 64 items.
//  3. keysets_union_kernel: one workgroup per tile of KS_TILE sorted items (ticket order).
//     The tile's keys and set numbers are staged in LDS; an item whose predecessor holds
//     another key heads a run; the heads are counted, a block scan and the decoupled look-back
//     give each head its place in the union, and the head's thread ORs 1 << set over its run.
//     A run that passes the tile's end is followed into the next tiles' items in global
//     memory (they were written by the launch before: no hand-off inside this one).
//
// No step depends on how the keys are distributed: the radix sort's tiles are cut by item
// count, never by key range, and so are this kernel's.  There is no bucket that can overflow
// and therefore no overflow path; the cost of a skewed key space is only the digit passes the
// sort cannot skip.
//
// Budget (keysets_union_kernel): 256 threads, LDS 8 B x (KS_TILE + 1) keys + KS_TILE set bytes
// + the scan words = 9.3 KB, so LDS never limits residency below the 8 workgroups of 4 waves a
// CU holds; the kernel keeps a key, a mask, four head flags and a few indices per thread, far
// below the 128 VGPRs at which a 4-wave workgroup still fills a SIMD 4 deep.
#include "dg_launch.h"

namespace dg {

namespace {

constexpr int UB = KS_BLOCK, UI = KS_ITEMS, UT = KS_TILE;

__global__ __launch_bounds__(UB) void keysets_gather_kernel(const KsSeg* segs, int k, u64 m, u64* cat,
                                                            uint8_t* set, u32* bad) {
  __shared__ const u64* s_keys[KS_MAX_K];
  __shared__ u64 s_off[KS_MAX_K + 1];
  for (int j = threadIdx.x; j <= k; j += UB) {
    if (j < k) s_keys[j] = segs[j].keys;
    s_off[j] = segs[j].off;
  }
  __syncthreads();
  bool unordered = false;
  for (u64 p = (u64)blockIdx.x * UB + threadIdx.x; p < m; p += (u64)gridDim.x * UB) {
    int a = 0, b = k;  // the last keyset j with s_off[j] <= p (empty keysets share an offset)
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (s_off[mid] <= p)
        a = mid;
      else
        b = mid;
    }
    const u64* kj = s_keys[a];
    const u64 i = p - s_off[a];
    const u64 key = kj[i];
    if (i > 0 && kj[i - 1] >= key) unordered = true;
    cat[p] = key;
    set[p] = (uint8_t)a;
  }
  if (unordered) atomicOr(bad, 1u);
}

// The same items in sorted order WITHOUT a sort, for a few thousand of them
// (dg_join_deltas_keyed's small batches, where the radix sort's eight passes are latency, not
// work): every keyset is ascending, so item (key x of keyset a) stands at
//   pos = Σ_t |{y in K_t : y < x}| + |{t < a : x in K_t}|
// among all items ordered by (key, keyset) -- k lower bounds per item, the searches of
// RANK_G keysets interleaved so that their loads are in flight together.  skey[pos] = x,
// sset[pos] = a: what the gather and the sort leave, with idx the identity.  A keyset that is
// not strictly ascending sets *bad (its items' places are then not a permutation: a place past
// the end is not written, and the caller discards the result).
constexpr int RANK_G = 8;
__global__ __launch_bounds__(UB) void keysets_rank_kernel(const KsSeg* segs, int k, u64 m, u64* skey, uint8_t* sset,
                                                          u32* bad) {
  __shared__ const u64* s_keys[KS_MAX_K];
  __shared__ u64 s_off[KS_MAX_K + 1];
  for (int j = threadIdx.x; j <= k; j += UB) {
    if (j < k) s_keys[j] = segs[j].keys;
    s_off[j] = segs[j].off;
  }
  __syncthreads();
  const u64 p = (u64)blockIdx.x * UB + threadIdx.x;
  if (p >= m) return;
  int a = 0, b = k;  // the last keyset j with s_off[j] <= p (empty keysets share an offset)
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (s_off[mid] <= p)
      a = mid;
    else
      b = mid;
  }
  const u64 i = p - s_off[a];
  const u64 x = s_keys[a][i];
  bool unordered = i > 0 && s_keys[a][i - 1] >= x;
  u64 pos = 0;
  for (int t0 = 0; t0 < k; t0 += RANK_G) {
    u64 lo[RANK_G], len[RANK_G], n[RANK_G];
    const u64* kt[RANK_G];
    u64 busy = 0;
#pragma unroll
    for (int g = 0; g < RANK_G; g++) {
      const int t = t0 + g < k ? t0 + g : t0;
      kt[g] = s_keys[t];
      n[g] = t0 + g < k ? s_off[t + 1] - s_off[t] : 0;
      lo[g] = 0;
      len[g] = n[g];
      busy |= len[g];
    }
    while (busy) {  // one step of every search: the group's loads go out together
      u64 v[RANK_G];
#pragma unroll
      for (int g = 0; g < RANK_G; g++) v[g] = len[g] ? kt[g][lo[g] + (len[g] >> 1)] : 0;
      busy = 0;
#pragma unroll
      for (int g = 0; g < RANK_G; g++) {
        const u64 half = len[g] >> 1;
        if (len[g]) {
          if (v[g] < x) {
            lo[g] += half + 1;
            len[g] -= half + 1;
          } else {
            len[g] = half;
          }
        }
        busy |= len[g];
      }
    }
    u64 eq[RANK_G];
#pragma unroll
    for (int g = 0; g < RANK_G; g++) eq[g] = (t0 + g < a && lo[g] < n[g]) ? kt[g][lo[g]] : ~x;
#pragma unroll
    for (int g = 0; g < RANK_G; g++) pos += lo[g] + (eq[g] == x ? 1u : 0u);
  }
  if (pos < m) {
    skey[pos] = x;
    sset[pos] = (uint8_t)a;
  } else {
    unordered = true;
  }
  if (unordered) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UB) void keysets_union_kernel(const u64* cat, const uint8_t* set, const u32* idx,
                                                           u64 m, u64 ntiles, u64* ukeys_d, u64* ukeys,
                                                           u64* masks, u64 cap, Scan scan, u64* d_count) {
  __shared__ u64 s_key[UT + 1];  // s_key[i + 1]: the tile's item i; s_key[0]: the item before the tile
  __shared__ uint8_t s_set[UT];
  __shared__ u32 s_wave[UB / WAVE + 1];
  __shared__ u64 s_b[2];
  if (threadIdx.x == 0) {
    const u32 t = atomicAdd(scan.ticket, 1u);
    if ((u64)t == ntiles - 1) atomicExch(scan.ticket, 0u);
    s_b[0] = t;
  }
  __syncthreads();
  const u64 tile = s_b[0];
  const u64 i0 = tile * UT;
  const u32 nt = (u32)min<u64>(UT, m - i0);
#pragma unroll
  for (int q = 0; q < UI; q++) {
    const u32 li = q * UB + threadIdx.x;
    if (li < nt) {
      const u64 p = idx ? idx[i0 + li] : i0 + li;
      s_key[li + 1] = cat[p];
      s_set[li] = set[p];
    }
  }
  if (threadIdx.x == 0) s_key[0] = tile ? cat[idx ? idx[i0 - 1] : i0 - 1] : 0;
  __syncthreads();
  // the heads among this thread's UI consecutive items
  const u32 l0 = threadIdx.x * UI;
  bool head[UI];
  u32 c = 0;
#pragma unroll
  for (int q = 0; q < UI; q++) {
    const u32 li = l0 + q;
    head[q] = li < nt && ((i0 + li) == 0 || s_key[li] != s_key[li + 1]);
    c += head[q] ? 1u : 0u;
  }
  u32 total;
  const u32 off = block_excl_scan<UB>(c, s_wave, &total);
  if (threadIdx.x < WAVE) {
    u64 prefix = 0;
    if (tile == 0) {
      if (threadIdx.x == 0) lb_publish(scan.state, 0, scan.epoch, LB_INC, total);
    } else {
      if (threadIdx.x == 0) lb_publish(scan.state, tile, scan.epoch, LB_AGG, total);
      prefix = lb_lookback(scan.state, tile, scan.epoch, scan.err);
      if (threadIdx.x == 0) lb_publish(scan.state, tile, scan.epoch, LB_INC, prefix + total);
    }
    if (threadIdx.x == 0) {
      s_b[1] = prefix;
      if (tile == ntiles - 1) d_count[0] = prefix + total;
    }
  }
  __syncthreads();
  u64 g = s_b[1] + off;
#pragma unroll
  for (int q = 0; q < UI; q++) {
    if (!head[q]) continue;
    const u32 li = l0 + q;
    const u64 key = s_key[li + 1];
    u64 mask = 0;
    u32 j = li;
    for (; j < nt && s_key[j + 1] == key; j++) mask |= 1ull << s_set[j];
    if (j == nt) {  // the run reaches the tile's end: its items in the tiles behind
      for (u64 gj = i0 + nt; gj < m; gj++) {
        const u64 p = idx ? idx[gj] : gj;
        if (cat[p] != key) break;
        mask |= 1ull << set[p];
      }
    }
    ukeys_d[g] = key;  // (g < m: no more heads than items)
    if (g < cap) {
      ukeys[g] = key;
      masks[g] = mask;
    }
    g++;
  }
}

}  // namespace

hipError_t launch_keysets_gather(const KsSeg* segs, int k, u64 m, u64* cat, uint8_t* set, u32* bad,
                                 hipStream_t st) {
  if (m == 0) return hipSuccess;
  u64 g = (m + UB * 4 - 1) / (UB * 4);
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(keysets_gather_kernel, dim3((unsigned)g), dim3(UB), 0, st, segs, k, m, cat, set, bad);
  return hipGetLastError();
}

hipError_t launch_keysets_rank(const KsSeg* segs, int k, u64 m, u64* skey, uint8_t* sset, u32* bad, hipStream_t st) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(keysets_rank_kernel, dim3((unsigned)((m + UB - 1) / UB)), dim3(UB), 0, st, segs, k, m, skey,
                     sset, bad);
  return hipGetLastError();
}

hipError_t launch_keysets_union(const u64* cat, const uint8_t* set, const u32* idx, u64 m, u64* ukeys_d,
                                u64* ukeys, u64* masks, u64 cap, const Scan& scan, u64* d_count,
                                hipStream_t st) {
  const u64 ntiles = ks_tiles(m);
  if (ntiles == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  hipLaunchKernelGGL(keysets_union_kernel, dim3((unsigned)ntiles), dim3(UB), 0, st, cat, set, idx, m, ntiles,
                     ukeys_d, ukeys, masks, cap, scan, d_count);
  return hipGetLastError();
}

}  // namespace dg
