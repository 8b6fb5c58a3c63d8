// join_twopass.hip — the join as two passes behind the partition launch, with no
// workgroup waiting on another: what a join re-runs on when the stream kernel's grid
// aborted for lack of residency (api_join.hip), and the A/B partner of the single pass
// (DG_JOIN_MODE=2).
// Pass 1 (join2_slot_kernel): one workgroup per tile stages the tile (dg_jtile.h),
// merges it, and writes its kept-row count and its compaction list (LDS slot numbers,
// u16).
// Pass 2 (join2_compact_kernel): each workgroup sums the counts before its tile and
// gathers the kept rows from a/b into the output.
#include "dg_arena.h"
#include "dg_jtile.h"

namespace dg {

namespace {

// LDS of one slot workgroup.  The VV tables are only read by the merge and the
// compaction list is only written after it (behind the block scan's barriers), so
// they share storage: the tile stays at 4 workgroups per CU.
struct TileLds {
  Buf buf;
  union {
    u64 tab[2][VT];
    unsigned short comp[JT];
  } u;
  u32 wave[JB / WAVE + 1];
};

template <bool FAST, bool KEYED>
__global__ __launch_bounds__(JB) void join2_slot_kernel(JoinArgs p) {
  __shared__ TileLds s;
  const int tid = threadIdx.x;
  const u64 total = p.a.n + p.b.n;
  if (FAST)
    for (int x = tid; x < 2 * VT; x += JB) (&s.u.tab[0][0])[x] = 0;
  const u64 t = blockIdx.x;
  const u64 a0 = p.splits[t], a1 = p.splits[t + 1];
  int nat, nbt;
  u64 b0;
  tile_geom(t, p.jt, a0, a1, total, &nat, &nbt, &b0);
  Staged r;
  issue_tile(p.a, p.b, nat, a0, b0, r);
  __syncthreads();  // zeroed tables visible
  if (FAST) fill_vv_tables(p.ca, p.cb, s.u.tab[0], s.u.tab[1]);
  commit_tile(r, s.buf);
  __syncthreads();
  u32 keep;
  unsigned short src[JI];
  const KeySlice ks{nullptr, p.keys, p.n_keys};
  merge_items<FAST, KEYED>(p.ca, p.cb, s.u.tab[0], s.u.tab[1], ks, p.b.n, s.buf, nat, nbt, a0, b0,
                           keep, src);
  u32 n;
  u32 pos = block_excl_scan<JB>(__popc(keep), s.wave, &n);  // barriers: tables dead
#pragma unroll
  for (int q = 0; q < JI; q++)
    if (keep & (1u << q)) s.u.comp[pos++] = src[q];
  __syncthreads();
  if (tid == 0) p.counts[t] = n;
  for (u32 q = tid; q < n; q += JB) p.lists[t * JT + q] = s.u.comp[q];
}

constexpr int CPB = 256;
constexpr int CPT = 8;  // counts loaded per thread per batch in the compact prologue

__global__ __launch_bounds__(CPB) void join2_compact_kernel(Rows a, Rows b, const u64* splits,
                                                            const unsigned short* lists,
                                                            const u32* counts, u64 ntiles,
                                                            RowsOut out, u64* d_count) {
  __shared__ u32 s_wave[CPB / WAVE + 1];
  __shared__ u64 s_pre;
  const u64 tile = blockIdx.x;
  // Σ counts[0, tile): every load of a batch is issued before the first add
  u64 part = 0;
  for (u64 base = 0; base < tile; base += (u64)CPB * CPT) {
    u32 v[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
      const u64 i = base + (u64)k * CPB + threadIdx.x;
      v[k] = i < tile ? counts[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < CPT; k++) part += v[k];
  }
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) part += __shfl_xor(part, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) s_wave[threadIdx.x / WAVE] = (u32)part;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 acc = 0;
    for (int w = 0; w < CPB / WAVE; w++) acc += s_wave[w];
    s_pre = acc;
    if (tile == ntiles - 1) d_count[0] = acc + counts[tile];
  }
  __syncthreads();
  const u64 base = s_pre, n = counts[tile];
  const u64 a0 = splits[tile], a1 = splits[tile + 1];
  const u64 d0 = tile * JT;
  const int nat = (int)(a1 - a0);
  const u64 b0 = d0 - a0;
  for (u64 q = threadIdx.x; q < n; q += CPB) {
    const int x = lists[tile * JT + q];
    const bool fb = x >= nat + 2;
    const u64 g = fb ? b0 - 1 + (u64)(x - nat - 2) : a0 - 1 + (u64)x;
    const Row r = load_row_sel(a, b, fb, g);
    store_row_nt(out, base + q, r);
  }
}

}  // namespace

hipError_t launch_two_pass(JoinArgs& p, bool fast, bool keyed, void* pass_tmp, hipStream_t st) {
  Arena arena(pass_tmp);
  const PassScratch l = pass_layout(arena, p.ntiles, JT);
  p.counts = l.counts;
  p.lists = l.lists;
  auto kern = fast ? (keyed ? join2_slot_kernel<true, true> : join2_slot_kernel<true, false>)
                   : (keyed ? join2_slot_kernel<false, true> : join2_slot_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)p.ntiles), dim3(JB), 0, st, p);
  hipLaunchKernelGGL(join2_compact_kernel, dim3((unsigned)p.ntiles), dim3(CPB), 0, st, p.a, p.b,
                     p.splits, p.lists, p.counts, p.ntiles, p.out, p.d_count);
  return hipGetLastError();
}

}  // namespace dg
