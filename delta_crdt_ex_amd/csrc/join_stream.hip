// join_stream.hip — the join's single pass (the default): join2_stream_kernel, a persistent
// grid of G resident workgroups (occupancy API) that walks the tiles statically, t = w + k*G,
// so tiles k*G .. k*G+G-1 form "stripe" k.  Per iteration a workgroup commits the tile it
// prefetched into registers to one of two LDS buffers, issues the loads of its next tile,
// merges JI positions per thread from LDS (keep/drop: dg_jtile.h), block-scans the keep
// flags into a u16 compaction list and publishes the tile's count as an {epoch, count}
// granule in a per-stripe array.  The tile is written out one iteration LATER: by then the
// G tiles before it have (nearly always) published their counts, so each workgroup sums
// those G counts itself (a 1-4 KB coalesced read) instead of chaining look-backs, and adds
// them to the offset of its previous tile (dg_jstripe.h).  Inputs are read once, outputs written
// once: 36 B x (N_in + N_out) of HBM traffic plus the splits' probes (dg_jsplit.h: from
// the partition launch, or searched by the kernel itself when launched fused, LATE).
// Here too: the grid's residency check, the 16 instantiations and their launch.
#include <mutex>

#include "dg_jsplit.h"
#include "dg_jstripe.h"
#include "dg_jtile.h"

namespace dg {

namespace {

#ifdef DG_STAMPS
// Diagnostic build only (DG_STAMPS=1): per-tile phase timestamps (s_memrealtime,
// 100 MHz) written by lane 0 into a buffer no other code reads.
__device__ u64 g_join_stamps[65536 * 16];
#define JSTAMP(tile, k)                                                              \
  do {                                                                               \
    __syncthreads();                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                               \
    if (threadIdx.x == 0 && (tile) < 65536) g_join_stamps[(tile) * 16 + (k)] =       \
        __builtin_amdgcn_s_memrealtime();                                            \
    __builtin_amdgcn_sched_barrier(0);                                               \
  } while (0)
// Slots 10 and 11 of a workgroup's first tile: where the hardware placed it (XCC_ID in
// the high word, HW_ID -- CU, SH, SE -- in the low one) and 1 + its blockIdx, so
// tools/stamps_report.py can say which workgroups share a CU.
#define JSTAMP_PLACE(tile)                                                                 \
  do {                                                                                     \
    if (threadIdx.x == 0 && (tile) < 65536) {                                              \
      g_join_stamps[(tile) * 16 + 10] =                                                    \
          ((u64)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32) |                         \
          (u64)__builtin_amdgcn_s_getreg((31 << 11) | 4);                                  \
      g_join_stamps[(tile) * 16 + 11] = (u64)blockIdx.x + 1;                               \
    }                                                                                      \
  } while (0)
#else
#define JSTAMP(tile, k) \
  do {                  \
  } while (0)
#define JSTAMP_PLACE(tile) \
  do {                     \
  } while (0)
#endif

// ------------------------------------------------------------- single-pass join
// join2_stream_kernel: persistent workgroups (the whole grid is co-resident: it is
// sized from the occupancy query); workgroup w merges tiles w, w + G, w + 2G, ...
// so iteration k of every workgroup together covers the stripe of tiles [kG, (k+1)G).
// Two LDS tile buffers alternate.  Iteration k of workgroup w (tile t = w + kG):
//   1. commit tile t's rows (prefetched into registers) to buffer k%2;
//   2. issue the loads of tile t + G into registers (they stream during the merge);
//   3. merge tile t, block-scan its keep bits: count n_t and compaction list;
//      publish n_t (an epoch-tagged 32-bit granule, written once), then issue the loads
//      of the G tile counts before tile t - G, those of tiles [t - 2G, t - G);
//   4. the offset of tile t - G: that of tile t - 2G plus those G counts.  They are the
//      counts of the workgroups BELOW w in stripe k-1 and of w and the workgroups above it
//      in stripe k-2 (dg_jstripe.h), so a workgroup waits for a prefix of the stripe it
//      writes and takes the stripe's total a stripe late: workgroup 0 never waits for the
//      current stripe, and one late workgroup holds up those above it, not the grid;
//   5. write tile t - G's kept rows (still in buffer (k-1)%2), coalesced, at that
//      offset.
// No look-back chain and no ticket: the counts below w were published one merge earlier
// and the others two, so step 4 rarely waits; its cost is one G-word read per iteration,
// issued behind the tile's own count.  Every wait points at a strictly earlier tile.  Spins
// stay bounded (scan.err bit 0 on timeout).
// (stripe_sums' partials are double-buffered by iteration parity, which drops the barrier
// a single buffer needs before its writes: measured neutral, config 5 356-360 vs 358-360 us
// and config 2 34.5-35.4 vs 34.6-34.7 us, rocprofv3 on one box; kept, one barrier fewer)

template <bool KEYED>
struct StreamLds {
  Buf buf[2];
  unsigned short comp[2][JT];
  u64 tab[2][VT];
  u64 kslice[2][KEYED ? KS : 1];    // keyed: the tile's keyset slice (<= KS entries)
  u64 kspl[KEYED ? 2 * FUSE_IT : 1];  // keyed + fused: keyset splits of this workgroup's tiles
  u32 wave[JB / WAVE + 1];
  u64 red[2][JB / WAVE];  // stripe_sums' wave partials, double-buffered by iteration parity
  u64 spl[2 * FUSE_IT];  // fused: splits of this workgroup's tiles (start, end per tile)
  u64 chk[JB / WAVE];    // CHG: each wave's last change event, and 1 + its lane (0: none)
  int chf[JB / WAVE];
  int vvfar;  // fused: whether a VV has an entry outside the tables (wave 0, fill_vv_wave0)
};

constexpr u32 CNT_BITS = 12;  // count field of a tile-count granule (JT < 4096)
static_assert(JT < (1 << CNT_BITS), "tile count must fit the granule's count field");

__device__ __forceinline__ void publish_count(u32* cs, u64 t, u32 epoch, u32 n) {
  __hip_atomic_store(cs + t, (epoch << CNT_BITS) | n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The G counts a workgroup awaits before it writes tile t, those of tiles [t - G, t)
// (dg_jstripe.h: the positions below its own in t's stripe, the rest of the stripe before),
// CQ per thread: issued behind the tile's own count (stripe_load), consumed after the
// barrier that follows (stripe_sums), which re-polls the ones not yet published and returns
// their sum, tile t's offset less that of the workgroup's previous tile.
struct StripeCounts {
  u32 v[CQ];
};

__device__ __forceinline__ void stripe_load(const u32* cs, u64 t, u64 G, StripeCounts& c) {
#pragma unroll
  for (int q = 0; q < CQ; q++) {
    // (every lane loads: one without a granule reads tile t's own; stripe_sums replaces
    // what it read -- here the select would wait for the load)
    const StripeSlot sl = stripe_slot(G, t, (u64)threadIdx.x + (u64)q * JB);
    c.v[q] = __hip_atomic_load(cs + sl.tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Waiting is safe only while the whole grid is resident.  Polls that go on for long
// check the start flags of the workgroups waited on: one that has started stays
// resident until it finishes, so the wait ends; one that has not (another stream's or
// process's kernels hold the CUs) makes the waiter raise the abort flag after
// ABORT_POLLS, and the grid runs on without waiting (err bit 2; the caller re-runs the
// join on the two-pass kernels).  Each workgroup stores its start flag once, at its stripe
// position: no contended counter at launch.
constexpr u32 ABORT_POLLS = 1u << 13;
constexpr int STAGGER_SLEEP = 10;  // s_sleep units (64 clocks each) per step of DG_JOIN_STAGGER

// The check's own arguments are read from the kernel-argument segment where they are
// used (volatile: not hoisted), so they hold no registers across the tile loop.
template <class T>
__device__ __forceinline__ T cold(const T* field) {
  return *(const volatile T*)field;
}

__device__ __forceinline__ const Scan* cold_scan() {
  return &((const JoinArgs*)__builtin_amdgcn_kernarg_segment_ptr())->scan;
}

// Whether this thread stops waiting: the grid has aborted, or (after ABORT_POLLS) a
// workgroup whose count it still lacks has not started.  (A lane without a granule holds
// the epoch's tag since stripe_sums replaced its value, so it lacks nothing.)
__device__ __forceinline__ bool grid_check(u32 epoch, u32 spins, u64 t, u64 G, const StripeCounts& c) {
  const Scan* sc = cold_scan();
  u32* abort = cold(&sc->abort);
  if (__hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) return true;
  if (spins <= ABORT_POLLS) return false;
  const u32* started = cold(&sc->started);
  bool absent = false;
#pragma unroll
  for (int q = 0; q < CQ; q++) {
    if ((c.v[q] >> CNT_BITS) == epoch) continue;
    const StripeSlot sl = stripe_slot(G, t, (u64)threadIdx.x + (u64)q * JB);
    if (__hip_atomic_load(started + stripe_position(G, sl.tile), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT) != epoch)
      absent = true;
  }
  if (!absent) return false;
  // (the epoch again from the argument segment: as a store's data it needs a vector
  // register, which the compiler otherwise sets aside before the tile loop and spills)
  __hip_atomic_store(abort, cold(&sc->epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicOr(cold(&sc->err), 2u);
  return true;
}

// After an abort the counts not yet published read as 0, so the rest of the grid runs
// through its tiles without waiting and writes stay inside the output (whose rows the
// caller discards).
__device__ __forceinline__ u64 stripe_sums(u32 epoch, u32* err, u64 t, u64 G, StripeCounts& c,
                                           u64* s_red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < CQ; q++)  // lanes without a granule count 0
    if (!stripe_slot(G, t, (u64)tid + (u64)q * JB).has) c.v[q] = epoch << CNT_BITS;
  for (u32 spins = 0;; spins++) {  // (rare) wait for counts not yet published
    bool ready = true;
#pragma unroll
    for (int q = 0; q < CQ; q++) ready &= (c.v[q] >> CNT_BITS) == epoch;
    if (ready) break;
    if ((spins & 63) == 63 && grid_check(epoch, spins, t, G, c)) {
#pragma unroll
      for (int q = 0; q < CQ; q++)
        if ((c.v[q] >> CNT_BITS) != epoch) c.v[q] = epoch << CNT_BITS;
      break;
    }
    if (spins > (1u << 24)) {  // unreachable on a co-resident grid
      atomicOr(err, 1u);
      break;
    }
    __builtin_amdgcn_s_sleep(2);
    // (the granules' address again from the argument segment, as grid_check reads its own:
    // the lane's address into the granules otherwise holds a register pair across the tile
    // loop for this rare path, which the keyed kernels with change events spill)
    const u32* cs_poll = cold(&cold_scan()->counts);
#pragma unroll
    for (int q = 0; q < CQ; q++)
      if ((c.v[q] >> CNT_BITS) != epoch)
        c.v[q] = __hip_atomic_load(cs_poll + stripe_slot(G, t, (u64)tid + (u64)q * JB).tile,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  u32 tot = 0;
#pragma unroll
  for (int q = 0; q < CQ; q++) tot += c.v[q] & ((1u << CNT_BITS) - 1);
  // (a wave's sum of <= 2 x 64 twelve-bit counts fits 32 bits: a DPP reduction)
  tot = wave_sum_u32(tot);
  constexpr int NW = JB / WAVE;
  // (no barrier before the writes: the caller alternates two s_red buffers by iteration
  // parity, and the previous reader of this buffer finished two iterations ago, behind the
  // iterations' own barriers)
  if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE] = tot;
  __syncthreads();
  u32 sum = 0;  // (<= CQ * JB counts below 2^CNT_BITS)
#pragma unroll
  for (int i = 0; i < NW; i++) sum += (u32)s_red[i];
  // (uniform, and said so: the offset it is added to then lives in scalar registers)
  return (u32)__builtin_amdgcn_readfirstlane((int)sum);
}

template <bool KEYED>
__device__ __forceinline__ void write_tile(const JoinArgs& p, const StreamLds<KEYED>& s, int bi,
                                           u64 o0, u32 n) {
  const Buf& b = s.buf[bi];
  for (u32 q = threadIdx.x; q < n; q += JB) {
    const Row x = lds_row(b, s.comp[bi][q]);
    store_row_nt(p.out, o0 + q, x);
  }
}

template <bool FAST, bool KEYED, bool CHG, bool LATE>
__global__ __launch_bounds__(JB) __attribute__((amdgpu_waves_per_eu(4, 8))) void join2_stream_kernel(JoinArgs p) {
  __shared__ StreamLds<KEYED> s;
  const int tid = threadIdx.x;
  const u64 total = p.a.n + p.b.n, ntiles = p.ntiles, w = blockIdx.x;
  const u64 G = gridDim.x - (LATE ? 1 : 0);  // tile workgroups
  u32* cs = p.scan.counts;  // tile-count granules
  const u32 epoch = p.scan.epoch;
  const Rows& A = p.a;
  const Rows& B = p.b;
  if (tid == 0)  // residency check (stripe_sums)
    __hip_atomic_store(p.scan.started + w, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (w < G) JSTAMP(w, 0);  // (stamps build: slot 0 of a workgroup's first tile = its entry)
  if (w < G) JSTAMP_PLACE(w);
  Staged r;
  u64 ga0 = 0, ga1 = 0;  // fused: the first tile's speculative splits
  // fused, version vectors: the VV tables are filled beside the split checks (dg_jtile.h)
  constexpr bool VV_EARLY = LATE && FAST && !KEYED;
  VvStaged vr;
  if (LATE) {
    if (w == G) {  // Dots.union(c1, c2) (aw_lww_map.ex:155), beside the tiles
      ctx_union_block<JB>(p.cu, s.wave);
      return;
    }
    // The VVs' entries are loaded ahead of the first tile: loads return in order, so the
    // wait for them is a counted one that leaves the tile's loads in flight.  (A scheduling
    // barrier: the compiler's scheduler would move them behind the tile's.)
    if (VV_EARLY) {
      issue_vv(p.ca, p.cb, A, B, vr);
      __builtin_amdgcn_sched_barrier(0);
    }
    // The first tile's loads go out at the proportional splits d * na / (na + nb) BEFORE
    // the exact search: replicas that hold the same keys (config 2) split exactly there,
    // so the tile streams in during the search (checked below; re-issued otherwise).
    {
      ga0 = split_guess(A.n, B.n, w * p.jt);
      ga1 = split_guess(A.n, B.n, min((w + 1) * p.jt, total));
      int gnat, gnbt;
      u64 gb0;
      tile_geom(w, p.jt, ga0, ga1, total, &gnat, &gnbt, &gb0);
      issue_tile(A, B, gnat, ga0, gb0, r);
    }
    // wave 0 writes the VV tables while the tile is in flight; the barrier behind the split
    // checks publishes them
    if (VV_EARLY && tid < WAVE && vv_in_wave(p.ca, p.cb)) {
      const bool far = fill_vv_wave0(vr, p.ca.n, p.cb.n, s.tab[0], s.tab[1]);
      if (tid == 0) s.vvfar = far;
    }
    // merge-path splits of this workgroup's (<= FUSE_IT) tiles: boundary q (tile q / 2,
    // side q % 2) by wave q mod the block's waves
    for (int q = tid / WAVE; q < 2 * FUSE_IT; q += JB / WAVE) {  // (wave-uniform)
      const u64 tk = w + (u64)(q >> 1) * G;
      if (tk >= ntiles) break;
      const u64 d = min((tk + (q & 1)) * p.jt, total);
      // the proportional split is checked first; the search runs only where it is not
      // exact.  (The check's loads are vector loads, q not being uniform to the compiler:
      // each waits for the tile's loads before it)
      const u64 g = split_guess(A.n, B.n, d);
      const u64 sp = guess_exact(A, B, d, g) ? g : mp_split(A, B, d);
      if ((tid & (WAVE - 1)) == 0) s.spl[q] = sp;
      if (KEYED) {
        const u64 kq = key_split(A, B, p.keys, p.n_keys, d, sp);
        if ((tid & (WAVE - 1)) == 0) s.kspl[q] = kq;
      }
    }
  }
  if (FAST && !VV_EARLY)
    for (int x = tid; x < 2 * VT; x += JB) (&s.tab[0][0])[x] = 0;
  if (LATE) __syncthreads();
  if (w < G) JSTAMP(w, 8);  // (stamps build: splits searched)
  // split of boundary `side` (0 start, 1 end) of the tile of iteration k.  The fused
  // launch is exactly the LATE kernel, so the choice between the LDS copy and the
  // partition's array is made at compile time: a run-time flag let the compiler merge the
  // two reads into one flat load, whose wait (vmcnt 0) drained the previous tile's output
  // stores on every iteration (A/B: config 5 0.375-0.379 vs 0.381-0.388 ms per join, config 2
  // 33-35 vs 34-36 us)
  auto split = [&](u64 tile, int k, int side) -> u64 {
    if (LATE) return s.spl[2 * k + side];
    return p.splits[tile + side];
  };
  // keyed: the keyset slice [kl, kl + km) of the tile of iteration k; its entries are
  // staged with the tile's rows (one per lane) when km <= KS
  auto kslice = [&](u64 tile, int k, u64* kl) -> u64 {
    u64 lo, hi;
    if (LATE) {
      lo = s.kspl[2 * k];
      hi = s.kspl[2 * k + 1];
    } else {
      lo = p.ksplits[tile];
      hi = p.ksplits[tile + 1];
    }
    *kl = lo;
    return min(hi + 1, p.n_keys) - lo;
  };
  u64 t = w;
  u64 a0 = split(t, 0, 0), a1 = split(t, 0, 1);
  // The partitioned kernel reads a tile's splits from the partition's array one iteration
  // before it issues the tile: read where they are used, their wait (a memory round trip)
  // stood before the tile's loads.  (Not the keyed kernels: they have no registers to
  // carry them in.)
  constexpr bool AHEAD = !LATE && !KEYED;
  u64 sa0 = 0, sa1 = 0;  // AHEAD: the splits of tile t + G
  auto splits_ahead = [&](u64 tile) {  // (clamped: the array has ntiles + 1 entries)
    const u64 tq = min(tile, ntiles - 1);
    sa0 = p.splits[tq];
    sa1 = p.splits[tq + 1];
  };
  if (AHEAD) splits_ahead(t + G);
  int nat, nbt;
  u64 b0;
  tile_geom(t, p.jt, a0, a1, total, &nat, &nbt, &b0);
  if (!LATE || a0 != ga0 || a1 != ga1) issue_tile(A, B, nat, a0, b0, r);  // (uniform)
  u64 kl = 0, km = 0, kk = 0;
  if (KEYED) {
    km = kslice(t, 0, &kl);
    if (km <= (u64)KS && (u64)tid < km) kk = p.keys[kl + tid];
  }
  if (!VV_EARLY) __syncthreads();  // zeroed tables visible
  if (w < G) JSTAMP(w, 9);  // (stamps build: first tile's loads issued)
  bool vv_far = false;
  if (VV_EARLY) {
    if (vv_in_wave(p.ca, p.cb)) {  // (uniform) filled by wave 0, before the barrier above
      vv_far = __builtin_amdgcn_readfirstlane(s.vvfar) != 0;
    } else {  // a VV of more than VT entries has one outside the tables: the merge with the
              // coverage search, and its tables filled as the partitioned kernel's are
      for (int x = tid; x < 2 * VT; x += JB) (&s.tab[0][0])[x] = 0;
      __syncthreads();
      vv_far = __syncthreads_or(fill_vv_tables(p.ca, p.cb, s.tab[0], s.tab[1]));
    }
  } else if (FAST) {
    vv_far = fill_vv_tables(p.ca, p.cb, s.tab[0], s.tab[1]);  // once per workgroup
    if (LATE) vv_far = __syncthreads_or(vv_far);
  }
  // DG_JOIN_STAGGER (default 0: measured and not kept): the upper half of the
  // stripe starts its tiles later by that many sleeps of about a quarter microsecond.  The
  // two workgroups of a CU are observed to sit in opposite halves (w and w + 256 on 256
  // CUs: speed only, nothing depends on it).  A bounded sleep: it waits on nothing, and
  // behind a long one the lower half meets the wait for the stripe before (the tests).
  if (2 * w >= G)  // (the upper half: `upper` below)
    for (int i = p.stagger; i > 0; i--)
      __builtin_amdgcn_s_sleep(STAGGER_SLEEP);
  u64 off = 0;  // output offset of this workgroup's previous tile (of tile w: the counts below it)
  u32 np = 0;    // kept rows of this workgroup's tile of the previous stripe
  // The two workgroups of a CU do not run at one pace: the upper half of every stripe
  // (observed: w + 256 sits beside w on 256 CUs) took 25 % longer per iteration, then ran its
  // last tiles alone on the CU.  Supposed, not measured: at equal priority the CU issues from
  // its older waves first, and the upper half is dispatched second.  The upper half raises
  // its waves' priority on every second iteration, which evens the two out (config 2
  // 31.9 -> 29.3-29.6 us per join, config 5 313 -> 285-291; always raised, the lower half
  // falls behind instead: 34.1-34.6).  Speed only: nothing depends on which workgroups share
  // a CU.
  const bool upper = 2 * w >= G;
  for (int k = 0;; k++) {
    const int bi = k & 1;
    if (upper) {
      if (k & 1)
        __builtin_amdgcn_s_setprio(1);
      else
        __builtin_amdgcn_s_setprio(0);
    }
    if (k > 0) JSTAMP(t, 0);
    JSTAMP(t, 1);
    commit_tile(r, s.buf[bi]);
    if (KEYED && km <= (u64)KS && (u64)tid < km) s.kslice[bi][tid] = kk;
    __syncthreads();
    JSTAMP(t, 2);
    const u64 tn = t + G;
    u64 a0n = 0, a1n = 0, b0n = 0, kln = 0, kmn = 0;
    int natn = 0, nbtn = 0;
    // the next tile's loads: issued before the merge, so they land while it runs.  (Until
    // round 6 the fused kernel issued them after its merge, measured faster then, 39 vs 42 us;
    // since the fused merge has no flat loads left (NOFB below) the early issue wins there
    // too: config 2 34.1-35.2 against 36.1-37.2 us per join, A/B on one box, three rounds.)
    auto issue_next = [&]() {
      a0n = AHEAD ? sa0 : split(tn, k + 1, 0);
      a1n = AHEAD ? sa1 : split(tn, k + 1, 1);
      // (sa0 / sa1 end here, before the load that refills them: while they overlapped it the
      // load went to other registers and was waited for at once, to be copied)
      if (AHEAD) asm volatile("" : "+v"(a0n), "+v"(a1n) : : "memory");
      tile_geom(tn, p.jt, a0n, a1n, total, &natn, &nbtn, &b0n);
      issue_tile(A, B, natn, a0n, b0n, r);
      if (AHEAD) splits_ahead(tn + G);
      if (KEYED) {
        kmn = kslice(tn, k + 1, &kln);
        // (the slice's start as a scalar: added to the lane's index first, the compiler
        // keeps p.keys + tid in a register pair across the loop, which the keyed kernels
        // with change events spill)
        const u64 kls = ((u64)__builtin_amdgcn_readfirstlane((int)(kln >> 32)) << 32) |
                        (u32)__builtin_amdgcn_readfirstlane((int)kln);
        if (kmn <= (u64)KS && (u64)tid < kmn) kk = (p.keys + kls)[tid];
      }
    };
    if (tn < ntiles) issue_next();
    JSTAMP(t, 7);
    u32 keep, ev = 0;
    unsigned short src[JI];
    const KeySlice ks{KEYED && km <= (u64)KS ? s.kslice[bi] : nullptr, p.keys + kl, km};
    // (fused joins whose VVs have no entry beyond the LDS tables -- every real replica set:
    // the merge without the global-memory coverage search, whose flat loads made each of
    // the merge's LDS waits also wait for the stripe counts in flight; config 2 35.7-37.5
    // against 36.3-39.6 us per join over three A/B sessions.  The partitioned kernel keeps
    // one merge: its copy without the search measured slower, 375-377 vs 340-367 us)
    if (LATE && FAST && !vv_far)
      merge_items<FAST, KEYED, CHG, true>(p.ca, p.cb, s.tab[0], s.tab[1], ks, B.n, s.buf[bi], nat,
                                          nbt, a0, b0, keep, src, &ev);
    else
      merge_items<FAST, KEYED, CHG>(p.ca, p.cb, s.tab[0], s.tab[1], ks, B.n, s.buf[bi], nat, nbt, a0,
                                    b0, keep, src, &ev);
    JSTAMP(t, 3);
    u32 n;
    u32 pos = block_excl_scan1<JB>(__popc(keep), s.wave, &n);  // (barriers before s.wave's next use)
#pragma unroll
    for (int q = 0; q < JI; q++)
      if (keep & (1u << q)) s.comp[bi][pos++] = src[q];
    if (tid == 0) publish_count(cs, t, epoch, n);
    // stripe k-1's counts: loaded here, behind this tile's own count, and in flight across
    // the barrier.  Loaded before the merge, beside the tile loads, they were read before the stripe's slower workgroups had published, and the re-poll
    // of stripe_sums (a sleep and a round trip per try) cost more than the overlap gave:
    // config 2 35.9-36.9 us per join before the tile loads and 37.5-37.7 after them, against
    // 33.0-34.0 after the merge and 33.5-33.8 here (parent 34.2-35.2; A/B on one box).
    // (With change events they are loaded behind that block, not held across it.)
    StripeCounts sc;
    if (!CHG && k > 0) stripe_load(cs, t - G, G, sc);
    __syncthreads();
    if (CHG) {  // the tile's change events (keys, ascending, repeats allowed) -> chg_tmp,
                // with the per-tile figures the changed-key kernels need (chg_sum/write)
      const Buf& cb = s.buf[bi];
      const int ne = __popc(ev);
      u64 fkey = 0, lkey = 0;
      u32 diff = 0;  // own events after this thread's first that differ from their predecessor
      bool seen = false;
#pragma unroll
      for (int q = 0; q < JI; q++)
        if (ev & (1u << q)) {
          const u64 k = buf_key(cb, src[q]);
          if (seen && k != lkey) diff++;
          if (!seen) fkey = k;
          lkey = k;
          seen = true;
        }
      // the event before this thread's first: a max-scan of (lane + 1, last event) over
      // the wave's lanes with events, then the nearest earlier wave with events
      // (DPP max-scan of the lane tags, then one shuffle for the key of the lane found)
      const int lane = tid & (WAVE - 1), wv = tid / WAVE;
      const u32 mi = wave_incl_max(ne ? (u32)lane + 1 : 0u);  // last lane <= this with events, + 1
      const u32 mx = wave_prev(mi);                            // ... < this lane
      const u64 pk = __shfl(lkey, mx > 0 ? (int)mx - 1 : 0, WAVE);
      const u32 ml = (u32)__builtin_amdgcn_readlane((int)mi, WAVE - 1);  // the wave's last
      const u64 wk = __shfl(lkey, ml > 0 ? (int)ml - 1 : 0, WAVE);
      if (lane == WAVE - 1) {
        s.chf[wv] = (int)ml;
        s.chk[wv] = wk;
      }
      int pm = (int)mx;
      u64 pkey = pk;
      __syncthreads();
      if (pm == 0)
        for (int w2 = wv - 1; w2 >= 0; w2--)
          if (s.chf[w2] > 0) {
            pm = 1;
            pkey = s.chk[w2];
            break;
          }
      if (ne && pm > 0 && fkey != pkey) diff++;
      // one scan for both: events (low 16 bits) and differing events (high 16 bits)
      u32 tot2;
      const u32 sc2 = block_excl_scan1<JB>((diff << 16) | (u32)ne, s.wave, &tot2);
      const u32 n2 = tot2 & 0xffffu, p0 = sc2 & 0xffffu;
      u64* dst = p.chg_tmp + t * (u64)JT;
      u32 p2 = p0;
#pragma unroll
      for (int q = 0; q < JI; q++)
        if (ev & (1u << q)) dst[p2++] = buf_key(cb, src[q]);
      if (tid == 0) {
        p.chg_cnt[t] = n2;
        p.chg_wu[t] = tot2 >> 16;
      }
      if (ne && p0 == 0) p.chg_fk[t] = fkey;
      if (ne && p2 == n2) p.chg_lk[t] = lkey;
      if (k > 0) stripe_load(cs, t - G, G, sc);
    }
    JSTAMP(t, 4);
    if (k > 0) {  // stripe k-1: this workgroup's tile t - G
      off += stripe_sums(epoch, p.scan.err, t - G, G, sc, s.red[k & 1]);
      JSTAMP(t, 5);
      write_tile(p, s, bi ^ 1, off, np);
    }
    JSTAMP(t, 6);
    np = n;
    if (tn >= ntiles) {
      StripeCounts last;  // its last tile: the same sum, a stripe earlier than the others'
      stripe_load(cs, t, G, last);
      off += stripe_sums(epoch, p.scan.err, t, G, last, s.red[(k + 1) & 1]);
      write_tile(p, s, bi, off, np);
      if (tid == 0 && t == ntiles - 1) p.d_count[0] = off + np;
      break;
    }
    t = tn;
    a0 = a0n;
    a1 = a1n;
    nat = natn;
    nbt = nbtn;
    b0 = b0n;
    kl = kln;
    km = kmn;
    __syncthreads();  // buffer bi^1 written out: free for the next commit
  }
}

}  // namespace

// The 16 instantiations: [FAST][KEYED][CHG][LATE].
StreamKernels stream_kernels(bool fast, bool keyed, bool chg) {
  static void (*const kerns[2][2][2][2])(JoinArgs) = {
      {{{join2_stream_kernel<false, false, false, false>, join2_stream_kernel<false, false, false, true>},
        {join2_stream_kernel<false, false, true, false>, join2_stream_kernel<false, false, true, true>}},
       {{join2_stream_kernel<false, true, false, false>, join2_stream_kernel<false, true, false, true>},
        {join2_stream_kernel<false, true, true, false>, join2_stream_kernel<false, true, true, true>}}},
      {{{join2_stream_kernel<true, false, false, false>, join2_stream_kernel<true, false, false, true>},
        {join2_stream_kernel<true, false, true, false>, join2_stream_kernel<true, false, true, true>}},
       {{join2_stream_kernel<true, true, false, false>, join2_stream_kernel<true, true, false, true>},
        {join2_stream_kernel<true, true, true, false>, join2_stream_kernel<true, true, true, true>}}}};
  return {kerns[fast][keyed][chg][0], kerns[fast][keyed][chg][1]};
}

// Workgroups of kernel `k` (JB threads) resident at once on the current device: the grid
// of a persistent kernel whose workgroups wait on each other.  Cached per (kernel, device):
// the occupancy query costs microseconds of host time on every launch otherwise.
u64 resident_grid(const void* k) {
  struct Entry {
    const void* k;
    int dev;
    u64 n;
  };
  static Entry cache[32];
  static int used = 0;
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  {
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < used; i++)
      if (cache[i].k == k && cache[i].dev == dev) return cache[i].n;
  }
  int per_cu = 0, cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, JB, 0) != hipSuccess || per_cu <= 0 ||
      cus <= 0)
    return 256;
  const u64 n = (u64)per_cu * (u64)cus;
  std::lock_guard<std::mutex> g(mu);
  if (used < 32) cache[used++] = {k, dev, n};
  return n;
}

// Launch of the persistent stream kernel.  Its workgroups wait on each other's tile
// counts, so the whole grid must be resident at once even while other kernels (another
// engine's join on another stream) compete for the CUs: a cooperative launch, which the
// runtime only dispatches as one co-resident grid (DG_JOIN_COOP=1; default: a plain
// launch).
hipError_t launch_stream(void (*kern)(JoinArgs), u64 grid, JoinArgs& p, hipStream_t st) {
  static const bool coop = [] {
    const char* v = getenv("DG_JOIN_COOP");
    return v && v[0] == '1';
  }();
  if (!coop) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(JB), 0, st, p);
    return hipGetLastError();
  }
  void* args[] = {&p};
  return hipLaunchCooperativeKernel((const void*)kern, dim3((unsigned)grid), dim3(JB), args, 0, st);
}

#ifdef DG_STAMPS
extern "C" int dg_debug_join_stamps(unsigned long long* host, size_t n) {
  if (n > 65536 * 16) n = 65536 * 16;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_join_stamps), n * 8) == hipSuccess ? 0 : -3;
}
#endif

}  // namespace dg
