// merkle_diff.hip — the whole-tree diff of two Merkle trees (dg_tree.h describes them) over
// their stores: the keys whose raw value maps differ, truncate_diff to max_sync_size
// (reference lib/delta_crdt/causal_crdt.ex:98,105,206-214).
//
// A workgroup per subtree of 4096 buckets; a subtree whose root matches is skipped,
// otherwise the workgroup descends it in strides of 4 levels (each thread owns 16 buckets
// and compares their ancestors 4 and 8 levels up, then the buckets only below differing
// ancestors: two round trips instead of twelve), locates each differing bucket's rows from
// the trees' per-bucket row counts, hashes just those rows and merges them key by key.
// count / write passes; keys past `cap` are counted, not written (max_sync_size truncation).
#include "dg_launch.h"
#include "dg_tree.h"

namespace dg {

namespace {

// ---------------------------------------------------------------- full diff
// One workgroup per subtree of 2^sub buckets (sub = min(depth, 12)), whose root sits at
// level Ls = depth - sub.
//  1. bounds: two waves of the subtree's workgroup find its first row in both stores
//     (a 64-ary wave lower bound: 4 dependent load rounds at 12.5M rows), beside the
//     descent's first loads (no separate launch).
//  2. count: a subtree whose roots match is skipped.  Otherwise the workgroup descends it
//     in strides of 4 levels.  Each thread owns 16 consecutive buckets: their ancestors
//     4 and 8 levels up (one node each), the subtree's root and the buckets' row counts
//     in both trees (u16) are loaded in one round trip, the 16 bucket nodes (the second
//     round trip) only where both ancestors differ.  (A level-by-level descent through a
//     frontier in LDS read 40 % fewer node bytes at 1 % differing keys but took 12 round
//     trips and 24 barriers: 281 us per config-4 diff.)  A block scan turns the row
//     counts into row ranges.  The
//     differing buckets' rows are listed and hashed by all threads at once (one round of
//     independent loads), and each thread merges its differing buckets' keys from LDS.
//     The subtree's differing keys go to scratch at (A start + B start) of the subtree,
//     unique and increasing across subtrees.  More rows than the LDS stage holds: each
//     thread merges its differing buckets over global memory instead.
//  3. write: each subtree's keys to their output offset, the keys past `cap` counted,
//     not written (truncation to max_sync_size).
constexpr int DB = DIFF_BLOCK;
constexpr u32 XSUB = 1u << DIFF_SUB;  // buckets per subtree (at most)
constexpr u32 OWN = XSUB / DB;        // buckets per thread
// DG_DIFF_NT (A/B only): the staged rows' columns read with non-temporal loads (1: every
// column, 2: all but the key).  Config-4 round (profiles/r6/ab_diff_take.txt): the count
// kernel 65.7 -> 49.9 us, but the round's next calls read the same rows -- the take B's,
// the keyed join A's -- and lose what the diff's cached loads left in L2 and the
// last-level cache: take_keys 40 -> 54 us, kd_count 52 -> 60 us, the round no faster;
// back to back 50.3 -> 52.0 us.  FETCH unchanged (114 MB).  Kept off.
#ifndef DG_DIFF_NT
#define DG_DIFF_NT 0
#endif
// rows of the differing buckets staged in LDS, differing buckets listed in LDS (the
// subtree's share of a 1 %-differing config-4 shard is ~1000 rows in ~120 buckets at 4096
// buckets, a quarter of that at 1024; a subtree beyond either merges over global memory)
constexpr u32 RCAP = XSUB >= 4096 ? 1664 : 640;
constexpr u32 DCAP = XSUB >= 4096 ? 512 : 160;
constexpr u32 NHD = 128;              // node term hashes staged per tree
#ifndef DG_DIFF_OCC
#define DG_DIFF_OCC 4
#endif
constexpr int DIFF_OCC = DG_DIFF_OCC;  // count workgroups per CU the kernel is compiled for
static_assert(OWN == 16 || OWN == 4, "a thread owns 16 or 4 buckets (32 or 8 bytes of counts per tree)");
constexpr u32 CW = OWN / 2;           // count words (two u16 halves) per thread and tree

struct DiffArgs {
  MerkleT ta, tb;
  Rows sa, sb;
  u64* out;
  u64 cap;
  u64* bnd;   // ntiles + 1 boundaries x 2 stores: first row of each subtree in A, then in B
  u64* cnt;   // differing keys per subtree
  u64* keys;  // scratch: nA + nB keys
  u64* bsum;  // per DB subtrees: the sum of their counts (zero when the count kernel starts)
  u64* bzero;  // the other parity's sums (the previous call's), zeroed by the write kernel
  u64 nzero;   // ... all of its words: a call of another depth may have used more of them
  u64 ntiles;
  u32 sub;
  u64* d_count;
};

// The take form (dg_merkle_diff_take): beside each differing key the count kernel stores
// where the key's run lies in the chosen store -- its first row in the low DIFF_LOC_LEN bits (a
// store holds fewer than 2^44 rows), its length above them (a bucket holds at most 65535;
// 0: the store lacks the key) -- and the subtree's sum of those lengths, kept as cnt / bsum
// are; the write kernel scans the lengths into offs and copies the rows.
struct DiffTakeArgs : DiffArgs {
  u64* loc;    // scratch: keys[x]'s run in the chosen store
  u64* rcnt;   // per subtree: the rows of its differing keys in the chosen store
  u64* rsum;   // per DB subtrees: the sum of their row counts (zero when the count kernel starts)
  u64* rzero;  // the previous take's sums, zeroed by the write kernel
  u64 nrzero;  // ... all of its words
  u32 side;    // 0: the rows of sa, 1: of sb
  u64* offs;   // cap + 1 row offsets
  RowsOut rows;
  u64 rcap;
};
template <bool TAKE>
using DiffP = std::conditional_t<TAKE, DiffTakeArgs, DiffArgs>;

// the counts of a thread's 16 buckets (u16) as 8 words of two halves: 32 bytes at
// c + first, one path for every subtree size (the counts array holds at least 16 entries,
// deltagpu.h); mask_counts16 zeroes what the thread does not own, AFTER the round trip's
// other loads are issued (any use of a loaded value -- a second load path for small
// subtrees, a mask -- makes the compiler wait for it right there)
__device__ __forceinline__ void load_counts16(const uint16_t* c, u32 first, u32 w[CW]) {
  if constexpr (OWN == 16) {
    const uint4* v = (const uint4*)(c + first);
    const uint4 x = v[0], y = v[1];
    w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w, w[4] = y.x, w[5] = y.y, w[6] = y.z, w[7] = y.w;
  } else {
    const uint2 x = *(const uint2*)(c + first);
    w[0] = x.x, w[1] = x.y;
  }
}
__device__ __forceinline__ void mask_counts16(u32 w[CW], u32 nb, bool owns) {
#pragma unroll
  for (u32 q = 0; q < CW; q++) {  // (nb < OWN: a tree of fewer buckets, thread 0's)
    const u32 keep = (2 * q + 1 < nb ? 0xFFFF0000u : 0u) | (2 * q < nb ? 0xFFFFu : 0u);
    w[q] &= owns ? keep : 0u;
  }
}

__device__ __forceinline__ u32 half16(const u32 w[CW], u32 i) { return (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; }

// a buffer descriptor over [base, base + bytes) for a wave-uniform base (the halves go
// through readfirstlane so the compiler can keep the descriptor in SGPRs; gfx950 flags)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rsrc(const u64* base, u32 bytes) {
  const u32 lo = __builtin_amdgcn_readfirstlane((u32)(uintptr_t)base);
  const u32 hi = __builtin_amdgcn_readfirstlane((u32)((uintptr_t)base >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
}
// one u64 through a descriptor; an offset past its range reads 0 without an access
__device__ __forceinline__ u64 buf_load_u64(__amdgpu_buffer_rsrc_t r, int off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
  return ((u64)v[1] << 32) | v[0];
}

#ifdef DG_STAMPS
// Diagnostic build only (DG_STAMPS=1): per-subtree phase timestamps (s_memrealtime) by
// thread 0 of each count workgroup, read back with dg_debug_diff_stamps
// (tools/diff_stamps.py).  Each stamp is behind a barrier, so only shares are meaningful.
__device__ u64 g_df_stamps[4096 * 8];
#define DSTAMP(k)                                                                    \
  do {                                                                               \
    __syncthreads();                                                                 \
    if (threadIdx.x == 0 && tile < 4096)                                             \
      g_df_stamps[tile * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                \
  } while (0)
#else
#define DSTAMP(k) \
  do {            \
  } while (0)
#endif

template <bool TAKE>
__global__ __launch_bounds__(DB, DIFF_OCC * DB / 256) void merkle_diff_count_kernel(DiffP<TAKE> p) {
  __shared__ u32 s_wave[DB / WAVE + 1];
  __shared__ u32 s_da[DCAP], s_db[DCAP];  // a differing bucket's first row in A / B (from the subtree's)
  __shared__ u32 s_dp[DCAP + 1];          // its first staged row
  __shared__ u32 s_dn[DCAP];              // its rows in A (high half) and B (low half)
  __shared__ u64 s_k[RCAP], s_h[RCAP];    // the staged rows' keys and row hashes
  __shared__ unsigned char s_rl[RCAP];     // bit 7: first row of a store's rows in its bucket;
                                           // at a key run's head, the run's length (< 127)
  __shared__ u64 s_nha[NHD], s_nhb[NHD];  // the trees' node term hashes (<= NHD nodes)
  const u32 depth = p.ta.depth, sub = p.sub, Ls = depth - sub, nb = 1u << sub;
  const u64 tile = blockIdx.x;
  const int tid = threadIdx.x;
  DSTAMP(0);
  const bool nha_lds = p.ta.th.on && p.ta.th.nn <= NHD, nhb_lds = p.tb.th.on && p.tb.th.nn <= NHD;
  const u64 root = ((1ull << Ls) - 1) + tile;
  const u64 nbnd = p.ntiles + 1;
  // ---- descent in strides of 4 levels: thread tid owns buckets [16 tid, 16 tid + 16) of
  //      the subtree, and their common ancestors 4 and 8 levels up (one node each) are
  //      loaded with the subtree's root, the owned buckets' row counts and the node term
  //      hashes in ONE round trip (every load unconditional at a clamped index, the
  //      unused ones selected away: a load under a divergent branch is waited for at the
  //      branch's join, one round trip each); the 16 bucket nodes only below differing
  //      ancestors, in a second one
  const bool owns = (u32)tid * OWN < nb;
  const u64 bucket0 = tile << sub;
  const u64 b0 = bucket0 + (u64)tid * OWN;  // the first owned bucket (tree-wide)
  const u64 b0c = owns ? b0 : bucket0;      // (clamped: the loads stay inside the subtree)
  const u64 ra = p.ta.nodes[root], rb = p.tb.nodes[root];
  const u64 gi = sub >= 8 ? ((1ull << (depth - 8)) - 1) + (b0c >> 8) : root;
  const u64 qi = sub >= 4 ? ((1ull << (depth - 4)) - 1) + (b0c >> 4) : root;
  const u64 ga = p.ta.nodes[gi], gb = p.tb.nodes[gi], qa = p.ta.nodes[qi], qb = p.tb.nodes[qi];
  u32 ca[CW], cb[CW];
  load_counts16(p.ta.counts + bucket0, owns ? (u32)tid * OWN : 0u, ca);
  load_counts16(p.tb.counts + bucket0, owns ? (u32)tid * OWN : 0u, cb);
  const u32 nna = nha_lds ? (u32)p.ta.th.nn : 0u, nnb = nhb_lds ? (u32)p.tb.th.nn : 0u;
  const u64 hna = nna ? p.ta.th.nh[(u32)tid < nna ? (u32)tid : 0u] : 0ull;
  const u64 hnb = nnb ? p.tb.th.nh[(u32)tid < nnb ? (u32)tid : 0u] : 0ull;
  // the subtree's first row in both stores: waves 0 and 1 look it up (the chunk index) or
  // search while the descent's loads are in flight (also for the write kernel, which
  // reads them from p.bnd)
  __shared__ u64 s_bnd[2];
  if (tid < 2 * WAVE) {
    const Rows& r = tid < WAVE ? p.sa : p.sb;
    const u64* st = tid < WAVE ? p.ta.starts : p.tb.starts;  // the trees' chunk index, if kept
    const u32 L1 = depth < MERKLE_UPL ? depth : MERKLE_UPL;
    // The chunk index describes the store the tree was built / updated against.  It is
    // trusted only when its end is this store's row count and the start lies inside the
    // store (wave-uniform: every lane reads the same two words); otherwise -- another store
    // handed to the diff, rows changed without a dg_merkle_update, or a shard tree over a
    // store that holds more shards -- the subtree's first row is searched, as without an
    // index, so a stale index never reads past the store or yields wrong keys.
    u64 x = 0;
    bool use_st = st != nullptr && sub >= L1;  // (a subtree smaller than an index chunk: searched)
    if (use_st) {
      x = st[(tile << sub) >> L1];
      use_st = st[1ull << (depth - L1)] == r.n && x <= r.n;
    }
    if (!use_st) x = wave_bucket_start(p.ta, r.key, r.n, tile << sub);
    if ((tid & (WAVE - 1)) == 0) {
      s_bnd[tid / WAVE] = x;
      p.bnd[(tid < WAVE ? 0 : nbnd) + tile] = x;
    }
  }
  static_assert(NHD <= DB, "one node term hash per thread");
  if ((u32)tid < nna) s_nha[tid] = hna;
  if ((u32)tid < nnb) s_nhb[tid] = hnb;
  if (ra == rb) {  // uniform: the whole subtree matches (the bounds are written anyway)
    if (tid == 0) {
      p.cnt[tile] = 0;
      if constexpr (TAKE) p.rcnt[tile] = 0;
    }
    return;
  }
  DSTAMP(1);
  u32 mine = 0;  // the owned buckets that differ (bit i: bucket 16 tid + i)
  const bool anc = owns && (sub < 8 || ga != gb) && (sub < 4 || qa != qb);
  if (nb >= (u32)(WAVE * OWN)) {
    // the wave's 64 x OWN buckets' nodes, loaded by the wave together: load i of a lane
    // reads node 64 i + lane (owner lane (64 i + lane) / OWN, only under its differing
    // ancestors), so each load instruction reads 512 contiguous bytes instead of one 8-B
    // node from each of 64 lines (a lane's own OWN nodes); every load is issued before any
    // compare, and the ballot of load i hands each of its 64 / OWN owner lanes its OWN bits
    // (buffer loads: a lane that must not load passes an offset past the descriptor's
    // range, which the hardware answers with 0 and no memory access -- a conditional
    // global load would be a branch, and the compiler waits for each load at its join)
    const int lane = tid & (WAVE - 1);
    const u64 amask = __ballot(anc);
    const u64 lv = ((1ull << depth) - 1) + (tile << sub) + (u64)(tid - lane) * OWN;
    const __amdgpu_buffer_rsrc_t na = wave_rsrc(p.ta.nodes + lv, WAVE * OWN * 8);
    const __amdgpu_buffer_rsrc_t nbr = wave_rsrc(p.tb.nodes + lv, WAVE * OWN * 8);
    u64 x[OWN], y[OWN];
    constexpr u32 OPL = WAVE / OWN;  // owner lanes per load
#pragma unroll
    for (u32 i = 0; i < OWN; i++) {
      const bool ld = (amask >> (OPL * i + lane / OWN)) & 1;
      const int off = ld ? (int)((64 * i + lane) * 8) : 0x7ffffff0;
      x[i] = buf_load_u64(na, off);
      y[i] = buf_load_u64(nbr, off);
    }
#pragma unroll
    for (u32 i = 0; i < OWN; i++) {
      const u64 bal = __ballot(x[i] != y[i]);
      if ((u32)lane / OPL == i) mine = (u32)(bal >> (OWN * (lane % OPL))) & ((1u << OWN) - 1);
    }
  } else if (anc) {  // a subtree of fewer than 1024 buckets: a thread loads its own nodes
    const u64 lv = ((1ull << depth) - 1) + b0;
    const u32 m = nb < OWN ? nb : OWN;
#pragma unroll
    for (u32 i0 = 0; i0 < OWN; i0 += 4) {
      u64 x[4], y[4];
#pragma unroll
      for (u32 i = 0; i < 4; i++) {
        x[i] = i0 + i < m ? p.ta.nodes[lv + i0 + i] : 0ull;
        y[i] = i0 + i < m ? p.tb.nodes[lv + i0 + i] : 0ull;
      }
#pragma unroll
      for (u32 i = 0; i < 4; i++) mine |= (x[i] != y[i] ? 1u : 0u) << (i0 + i);
    }
  }
  // ---- the differing buckets as a list (one entry per bucket, in bucket order): its rows'
  //      offsets in both stores (from the subtree's first row) and their place among the
  //      staged rows; then every per-bucket step runs one lane per differing bucket, not
  //      every thread over its 16 owned buckets (which ran each step masked 16 times)
  mask_counts16(ca, nb, owns);
  mask_counts16(cb, nb, owns);
  u32 ta_ = 0, tb_ = 0, rd = 0;
#pragma unroll
  for (u32 i = 0; i < OWN; i++) {
    const u32 x = half16(ca, i), y = half16(cb, i);
    ta_ += x;
    tb_ += y;
    if (mine >> i & 1u) rd += x + y;
  }
  // the four exclusive prefixes (rows in A, rows in B, staged rows, differing buckets) in
  // ONE barrier: four wave scans, the wave totals to LDS, each thread adds up the totals of
  // the waves before its own (4 waves) -- four block scans took 12 barriers
  constexpr int NW = DB / WAVE;
  __shared__ u32 s_w4[4 * NW];
  u32 offa, offb, slot0, d0, ND, R, TA, TB;
  {
    const u32 v[4] = {ta_, tb_, rd, (u32)__popc(mine)};
    u32 inc[4];
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
#pragma unroll
    for (int j = 0; j < 4; j++) inc[j] = wave_incl_scan(v[j]);
    if (lane == WAVE - 1)
#pragma unroll
      for (int j = 0; j < 4; j++) s_w4[j * NW + w] = inc[j];
    __syncthreads();
    u32 below[4], total[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      below[j] = total[j] = 0;
#pragma unroll
      for (int i = 0; i < NW; i++) {
        const u32 x = s_w4[j * NW + i];
        below[j] += i < w ? x : 0u;
        total[j] += x;
      }
    }
    offa = below[0] + inc[0] - v[0];
    offb = below[1] + inc[1] - v[1];
    slot0 = below[2] + inc[2] - v[2];
    d0 = below[3] + inc[3] - v[3];
    R = total[2];
    ND = total[3];
    TA = total[0];
    TB = total[1];
  }
  DSTAMP(2);
  const u64 a0 = s_bnd[0], c0 = s_bnd[1];  // (the barrier above came after the searches)
  if (a0 + TA > p.sa.n || c0 + TB > p.sb.n) {
    // (uniform) the trees count more rows here than the stores hold from the subtree's first
    // row: a store the tree does not describe.  No row is read past it and no key written;
    // the marker reaches the total, which the host reports as an input error.
    if (tid == 0) {
      p.cnt[tile] = DIFF_MISMATCH;
      if constexpr (TAKE) p.rcnt[tile] = 0;
      atomicAdd((unsigned long long*)&p.bsum[tile / DB], (unsigned long long)DIFF_MISMATCH);
    }
    return;
  }
  const bool lds = R <= RCAP && ND <= DCAP;  // uniform
  if (lds) {
    u32 d = d0, slot = slot0, ra = offa, rb = offb;
#pragma unroll
    for (u32 i = 0; i < OWN; i++) {
      const u32 x = half16(ca, i), y = half16(cb, i);
      if (mine >> i & 1u) {
        s_da[d] = ra;
        s_db[d] = rb;
        s_dp[d] = slot;
        s_dn[d] = (x << 16) | y;
        d++;
        slot += x + y;
      }
      ra += x;
      rb += y;
    }
    if (tid == 0) s_dp[ND] = R;
    __syncthreads();
    DSTAMP(3);
    // one lane per differing bucket writes, for each of the bucket's staged rows, the row's
    // place in its store into s_k (ROW_B: a row of B, ROW_FIRST: the first of its store's
    // rows in the bucket); the hashing step below reads that one word per row and
    // overwrites it with the row's key.  (Each row used to find its bucket by a binary
    // search of the LDS list: ~9 dependent LDS reads per row before its loads went out.)
    constexpr u64 ROW_B = 1ull << 63, ROW_FIRST = 1ull << 62;
    for (u32 e = tid; e < ND; e += DB) {
      const u32 sp = s_dp[e], xy = s_dn[e], x = xy >> 16, y = xy & 0xFFFFu;
      const u64 fa = a0 + s_da[e], fb = c0 + s_db[e];
      for (u32 r = 0; r < x; r++) s_k[sp + r] = (fa + r) | (r == 0 ? ROW_FIRST : 0ull);
      for (u32 r = 0; r < y; r++) s_k[sp + x + r] = (fb + r) | ROW_B | (r == 0 ? ROW_FIRST : 0ull);
    }
    __syncthreads();
    // hash the staged rows, all at once.  A thread's rows go in batches of RB: every column
    // load of the batch is issued before any row is hashed (one round trip per batch, not
    // one per row), and the node term hashes come from LDS (staged above), not from a
    // dependent global load.  A lane past the staged rows loads row 0 of a non-empty store
    // (its s_k entry may already hold another thread's key): no load sits under a
    // divergent branch, so all of them go out before any wait.
    const bool spare_b = p.sa.n == 0;
    constexpr int RB = 4;
    for (u32 u0 = 0; u0 < (RCAP + DB - 1) / DB; u0 += RB) {
      if (u0 * DB >= R) break;  // uniform
      u64 key[RB], val[RB], cnt[RB];
      i64 ts[RB];
      u32 nd[RB];
      bool fromb[RB];
      bool side0[RB];
#pragma unroll
      for (int j = 0; j < RB; j++) {
        const u32 q = (u0 + j) * DB + tid;
        {
          const u64 e = s_k[min(q, R - 1)];
          const bool in = q < R;
          fromb[j] = in ? (e & ROW_B) != 0 : spare_b;
          side0[j] = (e & ROW_FIRST) != 0;
          const Rows& S = fromb[j] ? p.sb : p.sa;
          const u64 i = in ? e & (ROW_FIRST - 1) : 0ull;
#if DG_DIFF_NT  // (A/B: non-temporal row loads, above)
          key[j] = DG_DIFF_NT == 2 ? S.key[i] : __builtin_nontemporal_load(S.key + i);
          val[j] = __builtin_nontemporal_load(S.val + i);
          ts[j] = __builtin_nontemporal_load(S.ts + i);
          nd[j] = __builtin_nontemporal_load(S.node + i);
          cnt[j] = __builtin_nontemporal_load(S.cnt + i);
#else
          key[j] = S.key[i];
          val[j] = S.val[i];
          ts[j] = S.ts[i];
          nd[j] = S.node[i];
          cnt[j] = S.cnt[i];
#endif
        }
      }
#pragma unroll
      for (int j = 0; j < RB; j++) {
        const u32 q = (u0 + j) * DB + tid;
        if (q < R) {
          const TermH& th = fromb[j] ? p.tb.th : p.ta.th;
          const u64* snh = fromb[j] ? s_nhb : s_nha;
          const bool lds_ok = fromb[j] ? nhb_lds : nha_lds;
          const u64 nt = lds_ok ? (nd[j] < (u32)th.nn ? snh[nd[j]] : (u64)nd[j]) : th_node(th, nd[j]);
          s_k[q] = key[j];
          s_h[q] = row_hash(key[j], th_val(th, val[j]), ts[j], nt, cnt[j]);
          s_rl[q] = side0[j] ? 0x80 : 0;
        }
      }
    }
    __syncthreads();
    // key runs, one thread per row: at the head of each run of equal keys within one
    // store's rows of a bucket, the run's leaf (its row hashes summed) replaces the head's
    // row hash and the run's length goes to s_rl's low bits (127: longer), so the merge
    // below takes one step per key with all of the step's reads independent.  (Only a
    // head's own thread writes its entries; the others read bit 7 and non-head rows.)
    // Diff 0.169 -> 0.178 of peak back to back, count kernel 68.3 -> 67.4 us in the
    // config-4 round (A/B; the merge used to walk every row with dependent LDS reads).
    for (u32 q = tid; q < R; q += DB) {
      const u64 k = s_k[q];
      if (!(s_rl[q] & 0x80) && s_k[q > 0 ? q - 1 : 0] == k) continue;  // not a head
      u64 sum = s_h[q];
      u32 x = q + 1;
      for (; x < R && !(s_rl[x] & 0x80) && s_k[x] == k; x++) sum += s_h[x];
      s_h[q] = sum;
      s_rl[q] = (unsigned char)((s_rl[q] & 0x80) | min(x - q, 127u));
    }
    __syncthreads();
    DSTAMP(4);
    // merge each differing bucket's keys (one lane per bucket) ONCE: a lane keeps its
    // first KR differing keys in registers, the block scan gives the offsets, and only a
    // lane with more keys than that merges its buckets a second time to write them all
    // (the merge used to run twice for every lane: count, then write)
    constexpr u32 KR = 4;
    u64 kr0 = 0, kr1 = 0, kr2 = 0, kr3 = 0;
    // (take form) the kept keys' located runs, and the lane's rows of its differing keys
    [[maybe_unused]] u64 lr0 = 0, lr1 = 0, lr2 = 0, lr3 = 0;
    [[maybe_unused]] u32 nrows = 0;
    auto merge = [&](bool write, u32 o) {
      u32 k2 = 0;
      // (a lane's buckets are contiguous, so the lanes' outputs in lane order are in
      // bucket order also when there are more differing buckets than lanes)
      const u32 per = (ND + DB - 1) / DB, d1 = min(ND, (tid + 1) * per);
      for (u32 d = tid * per; d < d1; d++) {
        const u32 na = s_dn[d] >> 16;
        u32 ia = s_dp[d], ie = ia + na, jb = ie, je = s_dp[d + 1];
        // (take form) a staged index of the chosen store's rows of this bucket + lbase = the
        // row's index in the store: from the bucket's list entry, once per bucket
        [[maybe_unused]] u64 lbase = 0;
        if constexpr (TAKE) lbase = p.side ? s_bnd[1] + s_db[d] - ie : s_bnd[0] + s_da[d] - ia;
        while (ia < ie || jb < je) {
          [[maybe_unused]] const u32 ia0 = ia, jb0 = jb;
          // (ia, jb sit on run heads; every read of the step at clamped indices, together)
          const u32 xa = min(ia, R - 1), xb = min(jb, R - 1);
          const u64 ka0 = s_k[xa], kb0 = s_k[xb], ha0 = s_h[xa], hb0 = s_h[xb];
          const u32 la = s_rl[xa] & 127u, lb = s_rl[xb] & 127u;
          const u64 ka = ia < ie ? ka0 : ~0ull, kb = jb < je ? kb0 : ~0ull;
          const u64 k = ka < kb ? ka : kb;
          const bool pa = ia < ie && ka == k, pb = jb < je && kb == k;
          const u64 ha = pa ? ha0 : 0ull, hb = pb ? hb0 : 0ull;
          if (pa) {
            if (la < 127u) ia += la;
            else for (; ia < ie && s_k[ia] == k; ia++) {}
          }
          if (pb) {
            if (lb < 127u) jb += lb;
            else for (; jb < je && s_k[jb] == k; jb++) {}
          }
          if (!(pa && pb) || ha != hb) {
            [[maybe_unused]] u64 lw = 0;
            if constexpr (TAKE) {  // (a run the store lacks: length 0 at the row it would sit at)
              const u32 len = p.side ? jb - jb0 : ia - ia0;
              lw = (lbase + (p.side ? jb0 : ia0)) | ((u64)len << DIFF_LOC_LEN);
              if (!write) nrows += len;
            }
            if (write) {
              p.keys[s_bnd[0] + s_bnd[1] + o + k2] = k;
              if constexpr (TAKE) p.loc[s_bnd[0] + s_bnd[1] + o + k2] = lw;
            } else {
              kr0 = k2 == 0 ? k : kr0;
              kr1 = k2 == 1 ? k : kr1;
              kr2 = k2 == 2 ? k : kr2;
              kr3 = k2 == 3 ? k : kr3;
              if constexpr (TAKE) {
                lr0 = k2 == 0 ? lw : lr0;
                lr1 = k2 == 1 ? lw : lr1;
                lr2 = k2 == 2 ? lw : lr2;
                lr3 = k2 == 3 ? lw : lr3;
              }
            }
            k2++;
          }
        }
      }
      return k2;
    };
    const u32 c = merge(false, 0);
    DSTAMP(5);
    u32 t2;
    u32 o;
    if constexpr (TAKE) {
      // keys and rows in one scan: neither exceeds the staged rows (R <= RCAP < 2^16)
      static_assert(RCAP < (1u << 16), "a subtree's staged keys and rows fit 16 bits each");
      u32 t;
      o = block_excl_scan<DB>(c | (nrows << 16), s_wave, &t) & 0xFFFFu;
      t2 = t & 0xFFFFu;
      if (tid == 0) {
        p.rcnt[tile] = t >> 16;
        if (t >> 16) atomicAdd((unsigned long long*)&p.rsum[tile / DB], (unsigned long long)(t >> 16));
      }
    } else {
      o = block_excl_scan<DB>(c, s_wave, &t2);
    }
    if (tid == 0) {
      p.cnt[tile] = t2;
      if (t2) atomicAdd((unsigned long long*)&p.bsum[tile / DB], (unsigned long long)t2);
    }
    if (c > KR) {
      merge(true, o);
    } else {
      // (the subtree's offset re-read from LDS: kept in registers through the kernel, it
      // spilled to scratch, and its reload waited for every store in flight)
      u64* dst = p.keys + (s_bnd[0] + s_bnd[1]) + o;
      if (c > 0) dst[0] = kr0;
      if (c > 1) dst[1] = kr1;
      if (c > 2) dst[2] = kr2;
      if (c > 3) dst[3] = kr3;
      if constexpr (TAKE) {
        u64* ldst = p.loc + (s_bnd[0] + s_bnd[1]) + o;
        if (c > 0) ldst[0] = lr0;
        if (c > 1) ldst[1] = lr1;
        if (c > 2) ldst[2] = lr2;
        if (c > 3) ldst[3] = lr3;
      }
    }
    DSTAMP(6);
    return;
  }
  // more differing rows or buckets than the LDS lists hold: each thread merges its owned
  // differing buckets over global memory
  u32 c = 0;
  [[maybe_unused]] u32 nrows = 0;  // (take form) the thread's rows of its differing keys
  for (int pass = 0; pass < 2; pass++) {
    u32 o = 0;
    if (pass == 1) {
      u32 t2;
      o = block_excl_scan<DB>(c, s_wave, &t2);
      if (tid == 0) {
        p.cnt[tile] = t2;
        if (t2) atomicAdd((unsigned long long*)&p.bsum[tile / DB], (unsigned long long)t2);
      }
      if constexpr (TAKE) {  // (a thread's 16 buckets hold < 2^20 rows, the subtree < 2^28)
        u32 rt;
        __syncthreads();  // s_wave is read until here
        block_excl_scan<DB>(nrows, s_wave, &rt);
        if (tid == 0) {
          p.rcnt[tile] = rt;
          if (rt) atomicAdd((unsigned long long*)&p.rsum[tile / DB], (unsigned long long)rt);
        }
      }
    }
    u32 k2 = 0, ra = offa, rb = offb;
    for (u32 i = 0; i < OWN; i++) {
      // (the counts re-read from memory: indexing the registers by a loop variable here
      // would put them in scratch for the whole kernel)
      const u64 bi = bucket0 + (u64)tid * OWN + i;
      const u32 x = bi - bucket0 < nb ? p.ta.counts[bi] : 0u, y = bi - bucket0 < nb ? p.tb.counts[bi] : 0u;
      if (mine >> i & 1u) {
        if constexpr (TAKE) {
          if (pass == 0)
            k2 += merge_bucket_loc<false>(p.sa, p.ta.th, a0 + ra, a0 + ra + x, p.sb, p.tb.th, c0 + rb,
                                          c0 + rb + y, nullptr, 0, nullptr, p.side, &nrows);
          else
            k2 += merge_bucket_loc<true>(p.sa, p.ta.th, a0 + ra, a0 + ra + x, p.sb, p.tb.th, c0 + rb,
                                         c0 + rb + y, p.keys + a0 + c0, o + k2, p.loc + a0 + c0, p.side, nullptr);
        } else if (pass == 0)
          k2 += merge_bucket<false, false>(p.sa, p.ta.th, a0 + ra, a0 + ra + x, p.sb, p.tb.th,
                                           nullptr, nullptr, c0 + rb, c0 + rb + y, nullptr, 0, 0);
        else
          k2 += merge_bucket<false, true>(p.sa, p.ta.th, a0 + ra, a0 + ra + x, p.sb, p.tb.th,
                                          nullptr, nullptr, c0 + rb, c0 + rb + y, p.keys + a0 + c0,
                                          o + k2, ~0ull);
      }
      ra += x;
      rb += y;
    }
    c = k2;
  }
}

#ifdef DG_STAMPS
}  // namespace
extern "C" int dg_debug_diff_stamps(unsigned long long* host, size_t n) {
  if (n > 4096 * 8) n = 4096 * 8;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_df_stamps), n * 8) == hipSuccess ? 0 : -3;
}
namespace {
#endif

// Scan and copy in one pass, one wave per tile: the tile's output offset is the sum of
// the earlier groups' tile sums (bsum, added by the count kernel: 256 same-word adds per
// group, no scan launch) plus the counts of the earlier tiles of its own group -- at
// most 255 + ntiles / 256 words, loaded by the 64 lanes at once -- then the lanes copy
// the tile's keys from scratch to the output below cap.  The last tile's wave writes
// the total.  Two round trips: every word the offset and the copy's source need is
// loaded at once (unconditional loads at clamped indices, the unused ones selected away),
// then the keys, all before any store.  (Loads in loops and under branches made it a
// chain of up to nine: count, group sums, the group's counts four times, bounds, keys
// twice.)
__global__ __launch_bounds__(WAVE) void merkle_diff_write_kernel(DiffArgs p) {
  // (subtree `tile`'s keys sit at bnd[tile] + bnd[ntiles + 1 + tile] in scratch)
  const int lane = threadIdx.x;
  const u64 tile = blockIdx.x, grp = tile / DB, g0 = grp * DB;
  if (tile == 0)  // the previous call's group sums: zero for the next call
    for (u64 x = lane; x < p.nzero; x += WAVE) p.bzero[x] = 0;
  const bool last = tile + 1 == p.ntiles;
  constexpr int CQ = DB / WAVE;
  const u64 n = p.cnt[tile];
  const u64 sa = p.bnd[tile], sb = p.bnd[p.ntiles + 1 + tile];
  u64 c[CQ];
#pragma unroll
  for (int q = 0; q < CQ; q++) {
    const u64 x = g0 + (u64)lane + (u64)q * WAVE;
    c[q] = p.cnt[x < tile ? x : tile];
  }
  const u64 b0 = p.bsum[(u64)lane < grp ? (u64)lane : 0ull];
  u64 before = (u64)lane < grp ? b0 : 0ull;
#pragma unroll
  for (int q = 0; q < CQ; q++) before += g0 + (u64)lane + (u64)q * WAVE < tile ? c[q] : 0ull;
  for (u64 x = lane + WAVE; x < grp; x += WAVE) before += p.bsum[x];  // (more than 64 groups)
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) before += __shfl_xor(before, d, WAVE);
  if (last && lane == 0) *p.d_count = before + n;
  // (no keys: an empty subtree, the count kernel's marker, a marker upstream, past cap)
  if (n == 0 || n == DIFF_MISMATCH || before >= DIFF_MISMATCH || before >= p.cap) return;
  const u64 src = sa + sb, m = n < p.cap - before ? n : p.cap - before;
  constexpr int KQ = 4;
  for (u64 x0 = 0; x0 < m; x0 += KQ * WAVE) {
    u64 k[KQ];
#pragma unroll
    for (int q = 0; q < KQ; q++) {
      const u64 x = x0 + (u64)q * WAVE + lane;
      k[q] = p.keys[src + (x < m ? x : m - 1)];
    }
#pragma unroll
    for (int q = 0; q < KQ; q++) {
      const u64 x = x0 + (u64)q * WAVE + lane;
      if (x < m) p.out[before + x] = k[q];
    }
  }
}

// The take form's write kernel: the same offsets, and beside the key offset a row offset out
// of rcnt / rsum by the same sums (every subtree before the one `cap` cuts is kept whole, so
// its row count is exact).  The wave then goes through the subtree's kept keys 64 at a time:
// a wave scan of the run lengths on top of the row offset gives offs, and the lanes copy the
// chunk's rows, four rows per lane in flight, each finding its key in the chunk's 64 offsets
// in LDS.  The subtree `cap` cuts -- or the last one when none is cut -- writes offs[kept] and
// the row total.  No key at or past cap and no row at or past rcap is written, and nothing
// where any subtree met a store its tree does not describe.
__global__ __launch_bounds__(WAVE) void merkle_diff_take_write_kernel(DiffTakeArgs p) {
  __shared__ u32 s_off[WAVE];
  __shared__ u64 s_row[WAVE];
  const int lane = threadIdx.x;
  const u64 tile = blockIdx.x, grp = tile / DB, g0 = grp * DB;
  if (tile == 0) {  // the previous calls' group sums: zero for the next ones
    for (u64 x = lane; x < p.nzero; x += WAVE) p.bzero[x] = 0;
    for (u64 x = lane; x < p.nrzero; x += WAVE) p.rzero[x] = 0;
  }
  const bool last = tile + 1 == p.ntiles;
  constexpr int CQ = DB / WAVE;
  const u64 n = p.cnt[tile];
  const u64 sa = p.bnd[tile], sb = p.bnd[p.ntiles + 1 + tile];
  u64 c[CQ], r[CQ];
#pragma unroll
  for (int q = 0; q < CQ; q++) {
    const u64 x = g0 + (u64)lane + (u64)q * WAVE;
    c[q] = p.cnt[x < tile ? x : tile];
    r[q] = p.rcnt[x < tile ? x : tile];
  }
  const u64 b0 = p.bsum[(u64)lane < grp ? (u64)lane : 0ull], r0 = p.rsum[(u64)lane < grp ? (u64)lane : 0ull];
  u64 before = (u64)lane < grp ? b0 : 0ull, rbefore = (u64)lane < grp ? r0 : 0ull;
#pragma unroll
  for (int q = 0; q < CQ; q++) {
    const bool in = g0 + (u64)lane + (u64)q * WAVE < tile;
    before += in ? c[q] : 0ull;
    rbefore += in ? r[q] : 0ull;
  }
  for (u64 x = lane + WAVE; x < grp; x += WAVE) before += p.bsum[x], rbefore += p.rsum[x];
  // every group's sum as well (the same words for up to 64 groups): a marker anywhere in the
  // tree, not only upstream, and this call writes nothing at all
  const u64 ng = (p.ntiles + DB - 1) / DB;
  const u64 a0 = p.bsum[(u64)lane < ng ? (u64)lane : 0ull];
  u64 all = (u64)lane < ng ? a0 : 0ull;
  for (u64 x = lane + WAVE; x < ng; x += WAVE) all += p.bsum[x];
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) {
    before += __shfl_xor(before, d, WAVE);
    rbefore += __shfl_xor(rbefore, d, WAVE);
    all += __shfl_xor(all, d, WAVE);
  }
  if (last && lane == 0) p.d_count[0] = before + n;
  if (all >= DIFF_MISMATCH) return;  // (the host reports the input error)
  // the subtree that writes offs[kept] and the row total: the one cap cuts, else the last
  const bool fin = (before <= p.cap && p.cap < before + n) || (last && before + n <= p.cap);
  const u64 m = before < p.cap ? (n < p.cap - before ? n : p.cap - before) : 0ull;  // keys kept here
  if (m == 0 && !fin) return;
  const Rows& S = p.side ? p.sb : p.sa;
  const u64 src = sa + sb;
  u64 rbase = rbefore;  // the row offset of the chunk's first key
  for (u64 x0 = 0; x0 < m; x0 += WAVE) {
    const u64 x = x0 + lane;
    const bool in = x < m;
    const u64 k = p.keys[src + (in ? x : m - 1)], w = p.loc[src + (in ? x : m - 1)];
    const u32 len = in ? (u32)(w >> DIFF_LOC_LEN) : 0u;
    const u32 inc = wave_incl_scan(len), T = (u32)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
    s_off[lane] = inc - len;
    s_row[lane] = w & ((1ull << DIFF_LOC_LEN) - 1);
    if (in) {
      p.out[before + x] = k;
      p.offs[before + x] = rbase + (inc - len);
    }
    __syncthreads();
    constexpr int RQ = 4;  // rows per lane in flight
    for (u32 q0 = 0; q0 < T; q0 += RQ * WAVE) {
      Row v[RQ];
#pragma unroll
      for (int q = 0; q < RQ; q++) {
        const u32 i = q0 + (u32)q * WAVE + lane, ic = i < T ? i : T - 1;
        u32 lo = 0;  // the last key of the chunk whose first row is at or before row ic
#pragma unroll
        for (u32 step = WAVE / 2; step >= 1; step >>= 1) lo += s_off[lo + step] <= ic ? step : 0u;
        v[q] = load_row(S, s_row[lo] + (ic - s_off[lo]));
      }
#pragma unroll
      for (int q = 0; q < RQ; q++) {
        const u32 i = q0 + (u32)q * WAVE + lane;
        const u64 dst = rbase + i;
        if (i < T && dst < p.rcap) {
          p.rows.key[dst] = v[q].key;
          p.rows.val[dst] = v[q].val;
          p.rows.ts[dst] = v[q].ts;
          p.rows.node[dst] = v[q].node;
          p.rows.cnt[dst] = v[q].cnt;
        }
      }
    }
    rbase += T;
    __syncthreads();  // (the next chunk overwrites the offsets)
  }
  if (fin && lane == 0) {
    if (p.offs) p.offs[before + m] = rbase;
    p.d_count[1] = rbase;
  }
}

}  // namespace

hipError_t launch_merkle_diff_take(const MerkleT& a, const Rows& sa, const MerkleT& b, const Rows& sb, u32 side,
                                   u64* out_keys, u64 cap, u64* offs, const RowsOut& rows, u64 rcap, u64* scratch,
                                   u64* bsum, u64* bsum_zero, u64* rsum, u64* rsum_zero, u64 nzero, u64 nrzero,
                                   u64* d_count, hipStream_t st) {
  DiffTakeArgs p;
  p.ta = a;
  p.tb = b;
  p.sa = sa;
  p.sb = sb;
  p.out = out_keys;
  p.cap = cap;
  p.ntiles = diff_tiles(a.depth);
  p.sub = diff_sub(a.depth);
  const DiffTakeScratch ts = diff_take_scratch(a.depth, sa.n, sb.n);
  p.bnd = scratch + ts.bnd;
  p.cnt = scratch + ts.cnt;
  p.keys = scratch + ts.keys;
  p.loc = scratch + ts.loc;
  p.rcnt = scratch + ts.rcnt;
  p.bsum = bsum;
  p.bzero = bsum_zero;
  p.rsum = rsum;
  p.rzero = rsum_zero;
  p.nzero = nzero;
  p.nrzero = nrzero;
  p.d_count = d_count;
  p.side = side;
  p.offs = offs;
  p.rows = rows;
  p.rcap = rcap;
  hipLaunchKernelGGL(merkle_diff_count_kernel<true>, dim3((unsigned)p.ntiles), dim3(DB), 0, st, p);
  hipLaunchKernelGGL(merkle_diff_take_write_kernel, dim3((unsigned)p.ntiles), dim3(WAVE), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_merkle_diff(const MerkleT& a, const Rows& sa, const MerkleT& b, const Rows& sb,
                              u64* out_keys, u64 cap, u64* scratch, u64* bsum, u64* bsum_zero, u64 nzero,
                              u64* d_count, hipStream_t st) {
  DiffArgs p;
  p.ta = a;
  p.tb = b;
  p.sa = sa;
  p.sb = sb;
  p.out = out_keys;
  p.cap = cap;
  p.ntiles = diff_tiles(a.depth);
  p.sub = diff_sub(a.depth);
  p.bnd = scratch;
  p.cnt = scratch + 2 * (p.ntiles + 1);
  p.keys = p.cnt + p.ntiles;
  p.bsum = bsum;  // zero: the write kernel of the call before zeroed it
  p.bzero = bsum_zero;
  p.nzero = nzero;
  p.d_count = d_count;
  // (the subtree bounds are searched inside the count kernel)
  hipLaunchKernelGGL(merkle_diff_count_kernel<false>, dim3((unsigned)p.ntiles), dim3(DB), 0, st, p);
  hipLaunchKernelGGL(merkle_diff_write_kernel, dim3((unsigned)p.ntiles), dim3(WAVE), 0, st, p);
  return hipGetLastError();
}

}  // namespace dg
