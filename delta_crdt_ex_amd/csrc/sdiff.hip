// sdiff.hip — the streaming diff of two stores: every key whose rows differ between `a`
// (old) and `b` (new), ascending, with -- per changed key -- the LWW read on either side
// (read/2, aw_lww_map.ex:211-224: the greatest ts, a tie going to the first row) and the
// key's rows in `b`.  It is what dg_join_deltas runs behind a fold of k deltas: the fold
// says nothing about which keys it changed, and a search per key (dg_take_keys,
// dg_read_diff) of a batch that touches half of a 10M-key state costs more than the fold.
//
// Both stores are streamed, all five columns compared; nothing is searched outside a tile.
// Four launches, none of which waits on another workgroup:
//
//  split  one thread per diagonal t * SDIFF_TILE of the merge of the two KEY columns: the
//         merge-path split, then the run of the key found there in both stores (galloping
//         from the split, so a run of any length costs its logarithm).  bounds[t] = the
//         run's first rows (lo) and the rows behind it (hi) in a and b.
//  count  one workgroup per diagonal.  Its tile is the boundary key's two runs, compared by
//         the whole workgroup (a run may be of any length), and the whole keys between
//         that run and the next diagonal's: fewer than SDIFF_TILE rows, their keys staged
//         in LDS (a's, then b's).  A thread per row: the head of a key's run finds the key's
//         run in the other store by a search of the staged keys and compares the rows.  A
//         key of `a` is owned by its head in a, a key of b alone by its head in b; a changed
//         key sets the bit of its owner's place in the merge of the two key columns, so the
//         set bits of the mask are the changed keys in ascending order.  Per tile: changed
//         keys and their rows in b.
//  scan   one workgroup: the tiles' offsets and the totals (d_counts[SD_KEYS], [SD_ROWS]).
//  write  one workgroup per tile that changed anything: the owners read their bit, a scan
//         over the tile's merge places gives every changed key its slot, and its thread
//         walks the two runs for the winners and copies the rows of b.
//
// A run that swallows several diagonals gives the same bounds at each: the first of them
// owns the run and the others are empty until the next key.  Keys 0 and 2^64 - 1 are keys
// like any other (no sentinel).  The stores must be sorted by the full tuple and unique
// (dg_store_check): equal row sets are then equal row sequences.
#include "dg_launch.h"

namespace dg {

namespace {

constexpr int SB = SDIFF_BLOCK;
constexpr u32 ST = (u32)SDIFF_TILE;
constexpr u32 MW = ST / 32 + 2;  // mask words a tile's places can touch
static_assert(ST == 4 * SB, "the write kernel scans four merge places per thread");
static_assert(ST <= 32768, "places, run lengths and their sums in 16 bits");
constexpr u64 NONE = ~0ull;

// first index <= pos of the run of K that ends at pos: k[i] <= K for every i < pos
__device__ __forceinline__ u64 run_lo(const u64* k, u64 pos, u64 K) {
  u64 step = 1, hi = pos;
  while (hi >= step && k[hi - step] == K) {
    hi -= step;
    step <<= 1;
  }
  u64 lo = hi >= step ? hi - step + 1 : 0;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (k[mid] < K)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// first index >= pos behind the run of K that starts at pos: k[i] >= K for every i >= pos
__device__ __forceinline__ u64 run_hi(const u64* k, u64 n, u64 pos, u64 K) {
  u64 step = 1, lo = pos;
  while (lo + step <= n && k[lo + step - 1] == K) {
    lo += step;
    step <<= 1;
  }
  u64 hi = lo + step <= n ? lo + step - 1 : n;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (k[mid] <= K)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sdiff_split_kernel(SdiffArgs p) {
  const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
  if (t > p.ntiles) return;
  const u64 na = p.a.n, nb = p.b.n, d = t * SDIFF_TILE;
  u64* o = p.bounds + 4 * t;
  if (d >= na + nb) {
    o[0] = o[2] = na;
    o[1] = o[3] = nb;
    return;
  }
  const u64 *ka = p.a.key, *kb = p.b.key;
  u64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {  // rows of a among the first d of the merge (a before b on equal keys)
    const u64 mid = (lo + hi) >> 1;
    if (ka[mid] <= kb[d - 1 - mid])
      lo = mid + 1;
    else
      hi = mid;
  }
  const u64 ia = lo, ib = d - lo;
  const bool va = ia < na, vb = ib < nb;  // (one of them holds: d < na + nb)
  const u64 xa = va ? ka[ia] : 0, xb = vb ? kb[ib] : 0;
  const u64 K = (va && vb) ? (xa < xb ? xa : xb) : (va ? xa : xb);
  o[0] = na ? run_lo(ka, ia, K) : 0;
  o[1] = nb ? run_lo(kb, ib, K) : 0;
  o[2] = na ? run_hi(ka, na, ia, K) : 0;
  o[3] = nb ? run_hi(kb, nb, ib, K) : 0;
}

// A tile: the boundary key's runs a[la0, ha) and b[lb0, hb) (`head`: this tile owns them)
// and the whole keys behind them, a[ha, ha + la) and b[hb, hb + lb).
struct Tile {
  u64 la0, lb0, ha, hb;
  u32 la, lb;
  bool head;
};

__device__ __forceinline__ Tile load_tile(const u64* bounds, u64 t) {
  const u64* c = bounds + 4 * t;
  const u64* q = bounds + 4 * (t ? t - 1 : 0);
  Tile x;
  x.la0 = c[0];
  x.lb0 = c[1];
  x.ha = c[2];
  x.hb = c[3];
  const u64 na0 = c[4], nb0 = c[5];
  x.head = t == 0 || q[0] != x.la0 || q[1] != x.lb0;
  const bool same = na0 == x.la0 && nb0 == x.lb0;  // the next diagonal lies in the same run
  const u64 la = (!same && na0 > x.ha) ? na0 - x.ha : 0, lb = (!same && nb0 > x.hb) ? nb0 - x.hb : 0;
  // fewer than ST rows between two diagonals when the stores are sorted; input that is not
  // must not overrun the staged keys
  x.la = (u32)(la < ST ? la : ST);
  x.lb = (u32)(lb < ST - x.la ? lb : ST - x.la);
  return x;
}

// the tile's keys into s_keys: a's, then b's
__device__ __forceinline__ void stage_keys(const SdiffArgs& p, const Tile& x, u64* s_keys) {
  const u64 *pa = opaque_ptr(p.a.key), *pb = opaque_ptr(p.b.key);
  for (u32 q = threadIdx.x; q < x.la + x.lb; q += SB) {
    const bool fb = q >= x.la;
    s_keys[q] = gload(fb ? pb : pa, fb ? x.hb + (q - x.la) : x.ha + q);
  }
}

// Row q of the staged keys.  owner: it is the head of its key's run and stands for the key
// (a's head when a has the key); ia / ib: the key's first rows among the tile's rows of a / b
// (lenA / lenB rows, 0: the store has not got the key); place: its place in the tile's merge.
struct Item {
  bool owner;
  u32 place, ia, ib, lenA, lenB;
};

__device__ __forceinline__ Item item_info(const u64* s_keys, u32 la, u32 lb, u32 q) {
  Item it{};
  const u64 key = s_keys[q];
  const bool fb = q >= la;
  const u32 own0 = fb ? la : 0, own1 = fb ? la + lb : la;  // this row's side, and the other
  const u32 oth0 = fb ? 0 : la, oth1 = fb ? la : la + lb;
  if (q != own0 && s_keys[q - 1] == key) return it;  // not a head
  u32 e = q + 1;
  while (e < own1 && s_keys[e] == key) e++;
  const u32 pos = (u32)lower_bound(s_keys, oth0, oth1, key);
  u32 f = pos;
  while (f < oth1 && s_keys[f] == key) f++;
  if (fb) {
    it.owner = f == pos;  // b alone has the key
    it.ia = pos;
    it.lenA = f - pos;
    it.ib = q - la;
    it.lenB = e - q;
  } else {
    it.owner = true;
    it.ia = q;
    it.lenA = e - q;
    it.ib = pos - la;
    it.lenB = f - pos;
  }
  it.place = it.ia + it.ib;
  return it;
}

__global__ __launch_bounds__(SB) void sdiff_count_kernel(SdiffArgs p) {
  __shared__ u64 s_keys[ST];
  __shared__ u32 s_mask[MW];
  __shared__ u32 s_cnt[2];
  const u32 tid = threadIdx.x;
  const u64 t = blockIdx.x;
  const Tile x = load_tile(p.bounds, t);
  for (u32 i = tid; i < MW; i += SB) s_mask[i] = 0;
  if (tid < 2) s_cnt[tid] = 0;
  stage_keys(p, x, s_keys);
  // the boundary key: its two runs row by row, by the whole workgroup
  const u64 hA = x.ha - x.la0, hB = x.hb - x.lb0;
  u32 hd = 0;
  if (x.head) {
    if (hA != hB) {
      hd = 1;
    } else {
      for (u64 r = tid; r < hA; r += SB) {
        const u64 i = x.la0 + r, j = x.lb0 + r;
        const u64 av = p.a.val[i], bv = p.b.val[j], ac = p.a.cnt[i], bc = p.b.cnt[j];
        const i64 at = p.a.ts[i], bt = p.b.ts[j];
        const u32 an = p.a.node[i], bn = p.b.node[j];
        hd |= (av != bv) | (at != bt) | (an != bn) | (ac != bc);
      }
    }
  }
  const u32 hchg = __syncthreads_or((int)hd) ? 1u : 0u;  // (and the staged keys are there)
  const u32 n = x.la + x.lb;
  const u64 p0 = x.ha + x.hb;          // the merge place of the tile's first staged row
  const u32 base = (u32)(p0 & 31);
  const bool both = p.a.n != 0 && p.b.n != 0;
  u32 nk = 0, nr = 0;
  for (u32 q0 = 0; q0 < n; q0 += SB) {
    const u32 q = q0 + tid;
    Item it{};
    if (q < n) it = item_info(s_keys, x.la, x.lb, q);
    bool chg = it.owner && it.lenA != it.lenB;  // (a key of one store alone: 0 rows in the other)
    const u32 m = (it.owner && !chg) ? it.lenA : 0;  // rows to compare
    if (both) {
      // every lane loads at a clamped index while any lane of the wave has rows left
      for (u32 r = 0; __any(r < m && !chg); r++) {
        const u32 rr = r < m ? r : (m ? m - 1 : 0);
        u64 i = x.ha + it.ia + rr, j = x.hb + it.ib + rr;
        i = i < p.a.n ? i : p.a.n - 1;
        j = j < p.b.n ? j : p.b.n - 1;
        const u64 av = p.a.val[i], bv = p.b.val[j], ac = p.a.cnt[i], bc = p.b.cnt[j];
        const i64 at = p.a.ts[i], bt = p.b.ts[j];
        const u32 an = p.a.node[i], bn = p.b.node[j];
        chg |= (r < m) & ((av != bv) | (at != bt) | (an != bn) | (ac != bc));
      }
    }
    if (chg) {
      atomicOr(&s_mask[(base + it.place) >> 5], 1u << ((base + it.place) & 31));
      nk++;
      nr += it.lenB;
    }
  }
  nk = wave_sum_u32(nk);
  nr = wave_sum_u32(nr);
  if ((tid & (WAVE - 1)) == 0 && nk) {
    atomicAdd(&s_cnt[0], nk);
    atomicAdd(&s_cnt[1], nr);
  }
  __syncthreads();
  // the mask is zero before the launch; a word at a tile's edge is shared with its neighbour
  for (u32 w = tid; w < MW; w += SB)
    if (s_mask[w]) atomicOr(&p.mask[(p0 >> 5) + w], s_mask[w]);
  if (tid == 0) {
    const u64 h0 = x.la0 + x.lb0;
    if (hchg) atomicOr(&p.mask[h0 >> 5], 1u << (h0 & 31));
    p.cnt_k[t] = (u64)s_cnt[0] + hchg;
    p.cnt_r[t] = (u64)s_cnt[1] + (hchg ? hB : 0);
  }
}

// the tiles' exclusive offsets and the totals, by one workgroup: a thread sums a stretch of
// tiles (u64: a boundary key may have any number of rows), the stretches are scanned
__global__ __launch_bounds__(1024) void sdiff_scan_kernel(SdiffArgs p) {
  __shared__ u64 s_w[2][1024 / WAVE + 1];
  const u32 tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const u64 T = p.ntiles, per = (T + 1023) / 1024;
  const u64 t0 = (u64)tid * per < T ? (u64)tid * per : T, t1 = t0 + per < T ? t0 + per : T;
  u64 sk = 0, sr = 0;
  for (u64 t = t0; t < t1; t++) {
    sk += p.cnt_k[t];
    sr += p.cnt_r[t];
  }
  u64 ik = sk, ir = sr;
  for (int d = 1; d < WAVE; d <<= 1) {
    const u64 yk = __shfl_up(ik, d), yr = __shfl_up(ir, d);
    if ((int)lane >= d) {
      ik += yk;
      ir += yr;
    }
  }
  if (lane == WAVE - 1) {
    s_w[0][w] = ik;
    s_w[1][w] = ir;
  }
  __syncthreads();
  if (tid == 0) {
    u64 rk = 0, rr = 0;
    for (int i = 0; i < 1024 / WAVE; i++) {
      const u64 a = s_w[0][i], b = s_w[1][i];
      s_w[0][i] = rk;
      s_w[1][i] = rr;
      rk += a;
      rr += b;
    }
    s_w[0][1024 / WAVE] = rk;
    s_w[1][1024 / WAVE] = rr;
  }
  __syncthreads();
  u64 ok = s_w[0][w] + ik - sk, orr = s_w[1][w] + ir - sr;
  for (u64 t = t0; t < t1; t++) {
    p.off_k[t] = ok;
    p.off_r[t] = orr;
    ok += p.cnt_k[t];
    orr += p.cnt_r[t];
  }
  if (tid == 0) {
    p.d_counts[SD_KEYS] = s_w[0][1024 / WAVE];
    p.d_counts[SD_ROWS] = s_w[1][1024 / WAVE];
  }
}

// read/1 of the run ts[r0, r0 + len) by the whole workgroup: the row of the greatest ts, the
// first of equal ones (NONE: len == 0).  Thread 0 has the result.
__device__ __forceinline__ u64 block_winner(const i64* ts, u64 r0, u64 len, i64* s_ts, u64* s_ix) {
  const u32 tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  u64 ix = NONE;
  i64 best = 0;
  for (u64 r = tid; r < len; r += SB) {
    const i64 v = ts[r0 + r];
    const bool take = ix == NONE || v > best;
    best = take ? v : best;
    ix = take ? r0 + r : ix;
  }
  for (int d = WAVE / 2; d; d >>= 1) {
    const i64 ov = __shfl_down(best, d);
    const u64 oi = __shfl_down(ix, d);
    const bool take = oi != NONE && (ix == NONE || ov > best || (ov == best && oi < ix));
    best = take ? ov : best;
    ix = take ? oi : ix;
  }
  __syncthreads();  // (the scratch of an earlier call is read by now)
  if (lane == 0) {
    s_ts[w] = best;
    s_ix[w] = ix;
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < SB / WAVE; i++) {
      const i64 ov = s_ts[i];
      const u64 oi = s_ix[i];
      const bool take = oi != NONE && (ix == NONE || ov > best || (ov == best && oi < ix));
      best = take ? ov : best;
      ix = take ? oi : ix;
    }
  }
  return ix;
}

__global__ __launch_bounds__(SB) void sdiff_write_kernel(SdiffArgs p) {
  __shared__ u64 s_keys[ST];
  __shared__ u32 s_pack[ST];  // per merge place: changed << 16 | the key's rows in b
  __shared__ unsigned short s_ia[ST], s_ib[ST], s_la[ST];
  __shared__ u32 s_mask[MW];
  __shared__ u32 s_wave[SB / WAVE + 1];
  __shared__ i64 s_ts[SB / WAVE];
  __shared__ u64 s_ix[SB / WAVE];
  const u32 tid = threadIdx.x;
  const u64 t = blockIdx.x;
  if (p.cnt_k[t] == 0) return;  // (the whole workgroup)
  u64 ok = p.off_k[t], orow = p.off_r[t];
  const bool wr = p.has_rows && p.d_counts[SD_ROWS] <= p.rows_cap;
  const Tile x = load_tile(p.bounds, t);
  const u64 p0 = x.ha + x.hb;
  const u32 base = (u32)(p0 & 31);
  stage_keys(p, x, s_keys);
  for (u32 i = tid; i < ST; i += SB) s_pack[i] = 0;
  for (u32 w = tid; w < MW; w += SB) s_mask[w] = p.mask[(p0 >> 5) + w];
  const u64 h0 = x.la0 + x.lb0;
  if (x.head && ((p.mask[h0 >> 5] >> (h0 & 31)) & 1)) {  // the boundary key changed
    const u64 hA = x.ha - x.la0, hB = x.hb - x.lb0;
    if (p.has_diffs) {
      const u64 wa = block_winner(p.a.ts, x.la0, hA, s_ts, s_ix);
      const u64 wb = block_winner(p.b.ts, x.lb0, hB, s_ts, s_ix);
      if (tid == 0 && ok < p.cap) {
        p.old_val[ok] = wa != NONE ? p.a.val[wa] : 0;
        p.new_val[ok] = wb != NONE ? p.b.val[wb] : 0;
        p.flags[ok] = (uint8_t)((hA ? KD_DIFF_OLD : 0u) | (hB ? KD_DIFF_NEW : 0u));
      }
    }
    if (tid == 0 && ok < p.cap) p.changed[ok] = hA ? p.a.key[x.la0] : p.b.key[x.lb0];
    if (wr)
      for (u64 r = tid; r < hB; r += SB) store_row(p.rows, orow + r, load_row(p.b, x.lb0 + r));
    ok += 1;
    orow += hB;
  }
  __syncthreads();
  const u32 n = x.la + x.lb;
  for (u32 q = tid; q < n; q += SB) {
    const Item it = item_info(s_keys, x.la, x.lb, q);
    const u32 bit = base + it.place;
    if (it.owner && ((s_mask[bit >> 5] >> (bit & 31)) & 1)) {
      s_pack[it.place] = 65536u | it.lenB;
      s_ia[it.place] = (unsigned short)it.ia;
      s_ib[it.place] = (unsigned short)it.ib;
      s_la[it.place] = (unsigned short)it.lenA;
    }
  }
  __syncthreads();
  u32 sum = 0;
#pragma unroll
  for (u32 j = 0; j < 4; j++) sum += s_pack[4 * tid + j];
  u32 total;
  u32 pre = block_excl_scan<SB>(sum, s_wave, &total);
  const bool need_b = wr || p.has_diffs;
#pragma unroll 1
  for (u32 j = 0; j < 4; j++) {
    const u32 place = 4 * tid + j, v = s_pack[place];
    const bool on = (v >> 16) != 0;
    const u32 lenB = on ? (v & 0xFFFFu) : 0, lenA = on ? s_la[place] : 0;
    const u32 ia = on ? s_ia[place] : 0, ib = on ? s_ib[place] : 0;
    const u64 kidx = ok + (pre >> 16), ridx = orow + (pre & 0xFFFFu);
    pre += v;
    const u64 key = on ? (lenA ? s_keys[ia] : s_keys[x.la + ib]) : 0;
    const u32 ma = p.has_diffs ? lenA : 0, mb = need_b ? lenB : 0;
    const u32 m = ma > mb ? ma : mb;
    i64 ta = 0, tb = 0;
    u64 va = 0, vb = 0;
    // every lane loads at a clamped index while any lane of the wave has rows left
    for (u32 r = 0; __any(r < m); r++) {
      if (p.has_diffs && p.a.n) {
        u64 i = x.ha + ia + (r < ma ? r : (ma ? ma - 1 : 0));
        i = i < p.a.n ? i : p.a.n - 1;
        const i64 ts = p.a.ts[i];
        const u64 val = p.a.val[i];
        const bool take = (r < ma) & ((r == 0) | (ts > ta));
        ta = take ? ts : ta;
        va = take ? val : va;
      }
      if (need_b && p.b.n) {
        u64 i = x.hb + ib + (r < mb ? r : (mb ? mb - 1 : 0));
        i = i < p.b.n ? i : p.b.n - 1;
        Row row = load_row(p.b, i);
        const bool take = (r < mb) & ((r == 0) | (row.ts > tb));
        tb = take ? row.ts : tb;
        vb = take ? row.val : vb;
        if (wr && r < mb) store_row(p.rows, ridx + r, row);
      }
    }
    if (on && kidx < p.cap) {
      p.changed[kidx] = key;
      if (p.has_diffs) {
        p.old_val[kidx] = va;
        p.new_val[kidx] = vb;
        p.flags[kidx] = (uint8_t)((lenA ? KD_DIFF_OLD : 0u) | (lenB ? KD_DIFF_NEW : 0u));
      }
    }
  }
}

}  // namespace

hipError_t launch_store_diff(const SdiffArgs& p, hipStream_t st) {
  if (p.ntiles == 0) return hipMemsetAsync(p.d_counts, 0, 2 * sizeof(u64), st);
  hipError_t rc = hipMemsetAsync(p.mask, 0, p.mask_words * sizeof(u32), st);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(sdiff_split_kernel, dim3((unsigned)((p.ntiles + 1 + 255) / 256)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(sdiff_count_kernel, dim3((unsigned)p.ntiles), dim3(SB), 0, st, p);
  hipLaunchKernelGGL(sdiff_scan_kernel, dim3(1), dim3(1024), 0, st, p);
  hipLaunchKernelGGL(sdiff_write_kernel, dim3((unsigned)p.ntiles), dim3(SB), 0, st, p);
  return hipGetLastError();
}

}  // namespace dg
