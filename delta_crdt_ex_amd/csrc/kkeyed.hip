// kkeyed.hip — the keyed fold of k deltas
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
// arrays are filled as kd_count_kernel (kdelta.hip) fills them with d = E: kd_finish_kernel and
// splice_kernel then write the state exactly as they do for one delta (the chain in
// kdelta.hip's header, with kk_count_kernel in kd_count_kernel's place).
//
// Per thread in LDS: each delta run's first row, length and cursor (a key may be in all 64
// keysets; 64 cursors do not fit registers), lane-major so that a wave's accesses to one
// delta's words fall on distinct banks.
#include "dg_hash.h"
#include "dg_kdcount.h"

namespace dg {

namespace {

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
  const u64 blk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
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
    key_run<KD_RUN>(p.a.key, p.a.n, k, a_lo, na);
    big = na > KD_RUN;
  }
  __syncthreads();  // (the staged runs)
  // the key's run in every delta whose keyset holds it
  for (u64 b = msk; b; b &= b - 1) {
    const u32 i = (u32)__builtin_ctzll(b);
    u64 lo;
    u32 n;
    key_run<KD_RUN>(s_run[i].key, s_run[i].n, k, lo, n);
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
    p.runs[u] = big ? 0ull : kd_run_pack(na, nn, ne, chg);
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
  // a delta row whose key is outside its delta's keyset: the keys' runs do not add up to the
  // deltas' rows; a node id the VV tables do not hold
  kd_count_tail(p, blk, v, [&](u64 n_d) { return n_d != q.e_rows || (*q.flag & KF_PREP_FAIL); });
}

__global__ __launch_bounds__(KDB) void kk_count_kernel(KkArgs q) { kk_count_body<false>(q); }
__global__ __launch_bounds__(KDB) void kk_count_diffs_kernel(KkArgs q) { kk_count_body<true>(q); }

}  // namespace

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
