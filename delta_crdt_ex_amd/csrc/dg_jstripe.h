// dg_jstripe.h — which tile counts a workgroup of join2_stream_kernel (join_stream.hip)
// awaits before it writes a tile, as plain index arithmetic that the host can compile too
// (tests/stripe_prefix.cc runs it for every workgroup of a grid).
//
// A grid of G workgroups walks the tiles in stripes: the workgroup at position x of the
// stripe merges tiles x, x + G, x + 2G, ...; tile x + sG is its tile of stripe s.  The
// output offset of that tile is
//
//   base_s + below_s,   below_s = Σ counts of positions [0, x) of stripe s
//   base_s = base_{s-1} + below_{s-1} + rest_{s-1},
//                       rest_{s-1} = Σ counts of positions [x, G) of stripe s - 1
//
// (stripe -1 counts 0), so a workgroup waits for the positions BELOW its own in the stripe
// it writes and takes the stripe's total one stripe late, from the counts of the stripe
// before, which were published a whole iteration earlier.  The G granules of the two parts
// are those of tiles [t - G, t), t = x + sG: contiguous, and every one of a strictly earlier
// tile.  base_{s-1} + below_{s-1} is the offset of the workgroup's own previous tile, so
// the kernel carries that one value and adds the G counts to it:
//
//   off(t) = off(t - G) + Σ counts of tiles [t - G, t) ∩ [0, t)
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DG_JSTRIPE_HD __host__ __device__ __forceinline__
#else
#define DG_JSTRIPE_HD inline
#endif

namespace dg {

// The granule that lane j (0 <= j, the kernel's tid + q * JB) loads for the write of tile t
// on a grid of G: `tile` is always inside [0, t] (a lane without a granule reads tile t's
// own, which its workgroup has published, and counts it 0); `low`: the granule counts into
// below_s (a position under x in the stripe of tile t), else into rest_{s-1}.
struct StripeSlot {
  uint64_t tile;
  bool has, low;
};

DG_JSTRIPE_HD StripeSlot stripe_slot(uint64_t G, uint64_t t, uint64_t j) {
  const bool has = j < G && t + j >= G;  // tile t + j - G exists (stripe -1 does not)
  StripeSlot s;
  s.tile = has ? t + j - G : t;
  s.has = has;
  s.low = has && s.tile >= t - t % G;
  return s;
}

// Stripe position of tile `tile` (the workgroup that publishes it: its start flag).
DG_JSTRIPE_HD uint64_t stripe_position(uint64_t G, uint64_t tile) { return tile % G; }

}  // namespace dg
