// join_changes.hip — dg_join2_changes: the keys whose rows the join changed (CausalCrdt's diff/3 after every join,
// causal_crdt.ex:343-351, over `keys`), ascending and unique, from the stream
// kernel's per-tile change events (ascending; a key repeats when several of its rows
// changed, possibly across tiles).  An event is kept where it differs from the event
// before it: inside its tile, or -- for a tile's first event -- the last event of the
// nearest non-empty earlier tile.  Every input is complete when these kernels run (the
// stream kernel wrote them), so nothing waits on another workgroup:
//   join2_stream_kernel<_, _, CHG>  per tile: its events, their count, the events that
//                     differ from their in-tile predecessor, the first and last event
//   chg_sum_kernel    per chunk of CCH tiles: the chunk's summary (below)
//   chg_write_kernel  per CWT tiles: its offset from the chunk summaries before it and the
//                     tiles of its own chunk before it, then one wave per tile writes the
//                     tile's kept events
// A summary of a run of tiles: the unique events the run would hold on its own, whether
// it has events, its first and last event.  Summaries combine associatively (the right
// run's first event repeats the left run's last one, or not), so any prefix is a
// reduction of a few of them.
// The scratch all three go through: chg_layout (dg_arena.h).
#include "dg_arena.h"
#include "dg_launch.h"

namespace dg {

namespace {

constexpr int JT = JOIN_TILE;  // events per tile (the stream kernel's tile)
constexpr int CCH = WAVE;  // tiles per chunk summary (one wave's)
constexpr int CB2 = 256;   // threads of the changed-key kernels
constexpr int CWT = CB2 / WAVE;  // tiles per chg_write_kernel workgroup: one per wave

struct ChgSum {
  u64 u;    // unique events of the run on its own
  u64 has;  // the run has events
  u64 fk, lk;
};
static_assert(CCH == CHG_CHUNK && sizeof(ChgSum) == CHG_SUM_BYTES, "chg_layout sizes the chunk summaries");

__device__ __forceinline__ ChgSum chg_combine(const ChgSum& L, const ChgSum& R) {
  if (!L.has) return ChgSum{L.u + R.u, R.has, R.fk, R.lk};
  if (!R.has) return L;
  return ChgSum{L.u + R.u - (R.fk == L.lk ? 1ull : 0ull), 1ull, L.fk, R.lk};
}

struct ChgArgs {
  const u64* ev;   // JT events per tile
  const u32* cnt;  // events per tile
  const u32* wu;   // events after the first that differ from their predecessor
  const u64* fk;   // the tile's first and last event (written when it has any)
  const u64* lk;
  ChgSum* chunk;   // per chunk of CCH tiles
  u64 ntiles;
  u64* out;
  u64 cap;
  u64* d_count;
};

__device__ __forceinline__ ChgSum chg_tile(const ChgArgs& p, u64 t) {
  const u32 n = p.cnt[t];
  if (n == 0) return ChgSum{0, 0, 0, 0};
  return ChgSum{(u64)p.wu[t] + 1, 1, p.fk[t], p.lk[t]};
}

// Ordered reduction of one summary per thread (thread order = tile order) over the block:
// shuffles down within each wave (lane 0 ends with its wave's run), then the waves in
// order.  Every thread returns the block's summary.
__device__ __forceinline__ ChgSum shfl_down_sum(const ChgSum& x, int d) {
  return ChgSum{__shfl_down(x.u, d, WAVE), __shfl_down(x.has, d, WAVE), __shfl_down(x.fk, d, WAVE),
                __shfl_down(x.lk, d, WAVE)};
}

__device__ ChgSum chg_block_reduce(ChgSum x, ChgSum* s_red) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const ChgSum y = shfl_down_sum(x, d);
    if (lane + d < WAVE) x = chg_combine(x, y);
  }
  if (lane == 0) s_red[wv] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    ChgSum r = s_red[0];
    for (int i = 1; i < CB2 / WAVE; i++) r = chg_combine(r, s_red[i]);
    s_red[CB2 / WAVE] = r;
  }
  __syncthreads();
  const ChgSum r = s_red[CB2 / WAVE];
  __syncthreads();
  return r;
}

// Summary of [t0, t1) (t1 - t0 <= WAVE) by one wave: one tile per lane, every lane
// returns it.
__device__ __forceinline__ ChgSum chg_wave_range(const ChgArgs& p, u64 t0, u64 t1) {
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 t = t0 + lane;
  ChgSum x = t < t1 ? chg_tile(p, t) : ChgSum{0, 0, 0, 0};
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const ChgSum y = shfl_down_sum(x, d);
    if (lane + d < WAVE) x = chg_combine(x, y);
  }
  return ChgSum{__shfl(x.u, 0, WAVE), __shfl(x.has, 0, WAVE), __shfl(x.fk, 0, WAVE),
                __shfl(x.lk, 0, WAVE)};  // lane 0's run, to every lane
}

// one wave per chunk of CCH tiles
__global__ __launch_bounds__(CB2) void chg_sum_kernel(ChgArgs p, u64 nchunk) {
  const u64 c = (u64)blockIdx.x * (CB2 / WAVE) + threadIdx.x / WAVE;
  if (c >= nchunk) return;  // (uniform per wave)
  const ChgSum r = chg_wave_range(p, c * CCH, min(c * CCH + CCH, p.ntiles));
  if ((threadIdx.x & (WAVE - 1)) == 0) p.chunk[c] = r;
}

__global__ __launch_bounds__(CB2) void chg_write_kernel(ChgArgs p) {
  __shared__ ChgSum s_red[CB2 / WAVE + 1];
  __shared__ ChgSum s_tile[CWT];
  __shared__ u64 s_off[CWT];
  __shared__ u32 s_dup[CWT];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const u64 t0 = (u64)blockIdx.x * CWT, chunk = t0 / CCH;
  // the prefix [0, t0): the chunk summaries before this chunk (CB2 at a time), then this
  // chunk's tiles before t0 (at most CCH - CWT of them)
  ChgSum acc{0, 0, 0, 0};
  for (u64 c0 = 0; c0 < chunk; c0 += CB2) {
    const ChgSum x = c0 + tid < chunk ? p.chunk[c0 + tid] : ChgSum{0, 0, 0, 0};
    acc = chg_combine(acc, chg_block_reduce(x, s_red));
  }
  // (wave 0: this chunk's tiles before t0; the block reduce's barriers above retired s_red)
  if (wv == 0) {
    const ChgSum in = chg_wave_range(p, chunk * CCH, t0);
    if (lane == 0) s_red[0] = chg_combine(acc, in);
  }
  if (tid < CWT) s_tile[tid] = t0 + tid < p.ntiles ? chg_tile(p, t0 + tid) : ChgSum{0, 0, 0, 0};
  __syncthreads();
  if (tid == 0) {  // this workgroup's tiles: offsets and first-event repeats, in order
    ChgSum run = s_red[0];
    for (int i = 0; i < CWT; i++) {
      const ChgSum x = s_tile[i];
      const bool dup = x.has && run.has && x.fk == run.lk;
      s_dup[i] = dup ? 1u : 0u;
      s_off[i] = run.u;
      run = chg_combine(run, x);
    }
    if (t0 + CWT >= p.ntiles) p.d_count[0] = run.u;  // the last workgroup: the total
  }
  __syncthreads();
  // one wave per tile: the tile's kept events at its offset (below cap)
  {
    const int i = wv;
    const u64 t = t0 + i;
    if (t >= p.ntiles) return;
    const u32 n = p.cnt[t];
    const u64* ev = p.ev + t * (u64)JT;
    u64 o = s_off[i];
    const bool dup0 = s_dup[i] != 0;
    for (u32 e0 = 0; e0 < n; e0 += WAVE) {
      const u32 e = e0 + lane;
      const u64 k = e < n ? ev[e] : 0;
      const bool keep = e < n && (e > 0 ? ev[e - 1] != k : !dup0);
      const u64 m = __ballot(keep);
      const u64 pos = o + __popcll(m & ((1ull << lane) - 1));
      if (keep && pos < p.cap) p.out[pos] = k;
      o += __popcll(m);
    }
  }
}

}  // namespace

hipError_t launch_join2_changes(u64 na, u64 nb, void* chg_tmp, u64* out, u64 cap, u64* d_count,
                                hipStream_t st) {
  const u64 ntiles = join2_tiles(na, nb);
  if (ntiles == 0) return hipMemsetAsync(d_count, 0, sizeof(u64), st);
  Arena arena(chg_tmp);
  const ChgScratch l = chg_layout(arena, ntiles, JT);
  ChgArgs p;
  p.ev = l.ev;
  p.cnt = l.cnt;
  p.wu = l.wu;
  p.fk = l.fk;
  p.lk = l.lk;
  p.chunk = (ChgSum*)l.chunk;
  p.ntiles = ntiles;
  p.out = out;
  p.cap = cap;
  p.d_count = d_count;
  const u64 nchunk = (ntiles + CCH - 1) / CCH;
  if (nchunk > 1) {  // (the last chunk's summary is never read, nor written: chg_layout)
    const u64 nc = nchunk - 1;
    hipLaunchKernelGGL(chg_sum_kernel, dim3((unsigned)((nc + CB2 / WAVE - 1) / (CB2 / WAVE))),
                       dim3(CB2), 0, st, p, nc);
  }
  hipLaunchKernelGGL(chg_write_kernel, dim3((unsigned)((ntiles + CWT - 1) / CWT)), dim3(CB2), 0,
                     st, p);
  return hipGetLastError();
}

}  // namespace dg
