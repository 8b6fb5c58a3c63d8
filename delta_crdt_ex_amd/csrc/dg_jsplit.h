// dg_jsplit.h — the merge-path split of a join's tile boundaries: which a row the merged
// sequence's diagonal d falls on, and (keyed joins) which keyset entry.  One wave per
// boundary.  Used by join2_partition_kernel (join.hip), which searches every boundary in a
// launch of its own, and by the fused join2_stream_kernel (join_stream.hip), whose
// workgroups search the boundaries of their own tiles.
//
// Key ids are 64-bit hashes, so the key gap at the proportional split (one probe) lands
// within a few rows of the split and one 64-wide window round finishes it (~5 cache lines
// per array instead of a 21-step search); any key distribution stays exact through a
// 128-ary fallback search.
#pragma once
#include "dg_device.h"

namespace dg {

namespace {

// Merge-path predicate on diagonal `diag` over global memory: A[i] <= B[diag-1-i]
// (ties go to A).  Full rows are only loaded when the keys tie.
__device__ __forceinline__ bool mp_pred(const Rows A, const Rows B, u64 diag, u64 i) {
  u64 j = diag - 1 - i;
  u64 ka = A.key[i], kb = B.key[j];
  if (ka != kb) return ka < kb;
  return row_le(load_row(A, i), load_row(B, j));
}

constexpr int PB = 256;      // threads per partition block = 4 boundaries
constexpr int PK = 2 * WAVE;  // samples per search round (two per lane)

// One wave: first i in [lo, hi) with NOT mp_pred(i) (hi if none) by a 128-ary search.
__device__ u64 mp_search(const Rows A, const Rows B, u64 d, u64 lo, u64 hi) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int round = 0; round < 64 && hi > lo; round++) {
    const u64 span = hi - lo;
    bool f0, f1;  // lane l evaluates samples 2l and 2l+1
    if (span <= (u64)PK) {
      const u64 x0 = lo + 2 * lane, x1 = x0 + 1;
      f0 = x0 < hi && !mp_pred(A, B, d, x0);
      f1 = x1 < hi && !mp_pred(A, B, d, x1);
    } else {
      const u64 x0 = lo + (span * (u64)(2 * lane + 1)) / (PK + 1);
      const u64 x1 = lo + (span * (u64)(2 * lane + 2)) / (PK + 1);
      f0 = !mp_pred(A, B, d, x0);
      f1 = !mp_pred(A, B, d, x1);
    }
    const u64 m0 = __ballot(f0), m1 = __ballot(f1);
    int kf = PK;  // first false sample
    if (m0 | m1) {
      const int l0 = m0 ? __ffsll((long long)m0) - 1 : 64;
      const int l1 = m1 ? __ffsll((long long)m1) - 1 : 64;
      kf = (l0 <= l1) ? 2 * l0 : 2 * l1 + 1;
    }
    if (span <= (u64)PK) {
      return (u64)kf < span ? lo + kf : hi;
    } else if (kf == PK) {
      lo = lo + (span * (u64)PK) / (PK + 1) + 1;
    } else {
      const u64 nh = lo + (span * (u64)(kf + 1)) / (PK + 1);
      if (kf > 0) lo = lo + (span * (u64)kf) / (PK + 1) + 1;
      hi = nh;
    }
  }
  return lo;
}

// Merge-path split of diagonal d (= #A rows among the first d merged rows).
// A window of 64 consecutive candidates is decided in ONE round trip (one per lane,
// a ballot), first around the proportional guess d * na / (na + nb): replicas that share
// most keys (config 2) split there exactly.  If the window does not bracket the split,
// the key gap B.key[d-1-c] - A.key[c] at the window's middle c (in units of the 2^64
// key space; the rows were just loaded, so this is a cache hit) converts to a row shift
// of gap * na*nb / ((na+nb) * 2^64), which lands within a few rows for hashed keys, and
// the next window is decided there.  Three windows without a bracket fall back to the
// exact 128-ary search for any key distribution.
__device__ u64 mp_split(const Rows A, const Rows B, u64 d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 na = A.n, nb = B.n, total = na + nb;
  const u64 lo = d > nb ? d - nb : 0, hi = min(d, na);
  if (hi - lo <= (u64)PK) return mp_search(A, B, d, lo, hi);
  const double scale = (double)na * (double)nb / ((double)total * 18446744073709551616.0);
  u64 i = (u64)((double)d * (double)na / (double)total);
  i = min(max(i, lo), hi - 1);
  {  // the key gap at the proportional guess first (one scalar round trip): replicas that
     // differ (config 5: the guess is a median 342 rows off, 90 % of the boundaries needed
     // a second window) now bracket in the first.  Partition at config 5: 26.2 -> 20.4 us
    const double gap = (double)B.key[d - 1 - i] - (double)A.key[i];
    const double lim = (double)(hi - lo);
    double sft = gap * scale;
    sft = sft > lim ? lim : (sft < -lim ? -lim : sft);
    i64 ni = (i64)i + (i64)sft;
    ni = ni < (i64)lo ? (i64)lo : (ni > (i64)hi - 1 ? (i64)hi - 1 : ni);
    i = (u64)ni;
  }
  for (int r = 0; r < 3; r++) {
    // one candidate per lane: the gap-shifted guess is a median 11 rows off at config 5,
    // so 64-wide windows bracket as well as 128-wide ones and read half the keys
    // (partition 19.0 -> 16.9 us per config-5 join, rocprofv3 A/B)
    constexpr u64 PW = WAVE;
    u64 wlo = i > lo + PW / 2 ? i - PW / 2 : lo;
    const u64 whi = min(wlo + PW, hi);
    wlo = whi - PW > lo ? whi - PW : lo;
    const u64 x0 = wlo + lane;
    const u64 m0 = __ballot(x0 < whi && !mp_pred(A, B, d, x0));
    const u64 kf = m0 ? (u64)(__ffsll((long long)m0) - 1) : whi - wlo;
    // bracketed iff the first false is not at the window's low edge (unless that edge is
    // lo) and some candidate is false (unless the window reaches hi)
    if ((kf > 0 || wlo == lo) && (kf < whi - wlo || whi == hi)) return wlo + kf;
    const u64 c = (wlo + whi) / 2;
    const double gap = (double)B.key[d - 1 - c] - (double)A.key[c];
    double sft = gap * scale;
    const double lim = (double)(hi - lo);
    sft = sft > lim ? lim : (sft < -lim ? -lim : sft);
    i64 ni = (i64)c + (i64)sft;
    ni = ni < (i64)lo ? (i64)lo : (ni > (i64)hi - 1 ? (i64)hi - 1 : ni);
    i = (u64)ni;
  }
  return mp_search(A, B, d, lo, hi);
}

// The proportional split of diagonal d, d * na / (na + nb) clamped to the diagonal's
// range: exact for replicas that hold the same keys (config 2).
__device__ __forceinline__ u64 split_guess(u64 na, u64 nb, u64 d) {
  const u64 lo = d > nb ? d - nb : 0, hi = min(d, na);
  const u64 i = (u64)((double)d * (double)na / (double)(na + nb));
  return min(max(i, lo), hi);
}

// Whether g is diagonal d's split: A[g-1] <= B[d-g] and not A[g] <= B[d-1-g] (full tuples;
// at the diagonal's ends one side is vacuous).  Uniform indices: scalar loads.
__device__ __forceinline__ bool guess_exact(const Rows& A, const Rows& B, u64 d, u64 g) {
  const u64 lo = d > B.n ? d - B.n : 0, hi = min(d, A.n);
  bool ok = true;
  if (g > lo) ok = row_le(load_row(A, g - 1), load_row(B, d - g));
  if (g < hi) ok = ok && !row_le(load_row(A, g), load_row(B, d - 1 - g));
  return ok;
}

// Keyed joins: the first index of keys[0, n_keys) >= the key at merged position d (split
// s), by the calling wave.  Tile t's keys lie in [key(t*jt), key((t+1)*jt)], so the
// keyset entries they can match are [ksplit(t), ksplit(t+1)] (keys are unique).
__device__ __forceinline__ u64 key_split(const Rows& A, const Rows& B, const u64* keys, u64 n_keys,
                                         u64 d, u64 s) {
  const u64 ib = d - s;
  const bool va = s < A.n, vb = ib < B.n;
  if (!va && !vb) return n_keys;
  const u64 ka = va ? A.key[s] : ~0ull, kb = vb ? B.key[ib] : ~0ull;
  return wave_lower_bound(keys, n_keys, min(ka, kb));
}

}  // namespace

}  // namespace dg
