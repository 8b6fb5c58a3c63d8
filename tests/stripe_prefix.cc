// The stream join's stripe-count recurrence (csrc/dg_jstripe.h) on the host
// (tests/test_stripe_prefix.py builds this with ASan and UBSan and runs it).  For grids of
// G workgroups and tile counts that end in every kind of last stripe, every tile gets a
// random count in [0, JT]; every workgroup then walks its tiles as join2_stream_kernel
// does, loading through stripe_slot the granules of its lanes, and must arrive at the
// plain prefix sum over tiles: in the two-sum form (below_s, rest_{s-1}, base_s) and in the
// carried-offset form the kernel runs.  Every lane's granule must lie inside [0, ntiles),
// and the granules a write counts must be exactly those of tiles [t - G, t).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dg_jstripe.h"

using namespace dg;
typedef uint64_t u64;

static const u64 JT = 1016;     // JOIN_TILE (csrc/dg_launch.h)
static const u64 LANES = 1024;  // CQ * JB: the lanes of a workgroup's stripe_load

static int g_fail = 0;
static long g_checked = 0;
#define CHECK(c, ...)                               \
  do {                                              \
    g_checked++;                                    \
    if (!(c)) {                                     \
      if (g_fail++ < 20) {                          \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
    }                                               \
  } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// The two classes of the stagger: E holds the low G_E = ceil(G / 2) positions of a
// stripe, L the rest; position = class * G_E + index.
struct Place {
  int cls;
  u64 index;
};
static Place place_of(u64 G, u64 x) {
  const u64 ge = (G + 1) / 2;
  return x < ge ? Place{0, x} : Place{1, x - ge};
}

static void run(u64 G, u64 ntiles) {
  // the granules live in a block of exactly ntiles words: ASan sees a read outside it
  std::vector<uint32_t> count(ntiles);
  std::vector<u64> prefix(ntiles + 1, 0);
  for (u64 t = 0; t < ntiles; t++) {
    const u64 r = rng() % 8;
    count[t] = r == 0 ? 0 : r == 1 ? (uint32_t)JT : (uint32_t)(rng() % (JT + 1));
    prefix[t + 1] = prefix[t] + count[t];
  }
  const u64 ge = (G + 1) / 2;
  u64 total = ~0ull;
  std::vector<char> seen(G);
  for (u64 x = 0; x < G && x < ntiles; x++) {
    const Place pl = place_of(G, x);
    CHECK(pl.cls * ge + pl.index == x, "G=%llu x=%llu: class %d index %llu", (unsigned long long)G,
          (unsigned long long)x, pl.cls, (unsigned long long)pl.index);
    CHECK(pl.cls == 0 ? pl.index < ge : pl.index < G - ge, "G=%llu x=%llu: index outside its class",
          (unsigned long long)G, (unsigned long long)x);
    u64 off = 0;                          // the kernel's carried offset
    u64 base = 0, below = 0, rest_prev;  // the two-sum form: base_{s-1}, below_{s-1}
    for (u64 t = x, s = 0; t < ntiles; t += G, s++) {
      u64 below_s = 0, sum = 0, loaded = 0;
      rest_prev = 0;
      seen.assign(G, 0);
      for (u64 j = 0; j < LANES + 6; j++) {
        const StripeSlot sl = stripe_slot(G, t, j);
        CHECK(sl.tile < ntiles && sl.tile <= t, "G=%llu n=%llu t=%llu lane %llu loads tile %llu",
              (unsigned long long)G, (unsigned long long)ntiles, (unsigned long long)t,
              (unsigned long long)j, (unsigned long long)sl.tile);
        if (sl.tile >= ntiles) continue;
        const u64 n = count[sl.tile];  // (every lane loads)
        if (!sl.has) continue;
        CHECK(j < G && sl.tile < t && sl.tile + G >= t, "G=%llu t=%llu lane %llu counts tile %llu",
              (unsigned long long)G, (unsigned long long)t, (unsigned long long)j,
              (unsigned long long)sl.tile);
        const u64 pos = stripe_position(G, sl.tile);
        CHECK(!seen[pos], "G=%llu t=%llu: position %llu counted twice", (unsigned long long)G,
              (unsigned long long)t, (unsigned long long)pos);
        seen[pos] = 1;
        // below_s: positions under x of stripe s; rest_{s-1}: positions from x up of stripe s - 1
        CHECK(sl.low == (pos < x) && (sl.low ? sl.tile / G == s : sl.tile / G + 1 == s),
              "G=%llu t=%llu tile %llu: wrong sum", (unsigned long long)G, (unsigned long long)t,
              (unsigned long long)sl.tile);
        // a wait points at a strictly earlier tile; E (low positions) awaits no L count of
        // the stripe it writes
        if (pl.cls == 0 && sl.tile / G == s) CHECK(place_of(G, pos).cls == 0, "E waits for L");
        (sl.low ? below_s : rest_prev) += n;
        sum += n;
        loaded++;
      }
      CHECK(loaded == (t < G ? t : G), "G=%llu t=%llu: %llu granules counted", (unsigned long long)G,
            (unsigned long long)t, (unsigned long long)loaded);
      base = base + below + rest_prev;  // base_s (stripe -1 counts 0)
      below = below_s;
      off += sum;
      CHECK(base + below == prefix[t], "G=%llu n=%llu tile %llu: two-sum offset %llu, prefix %llu",
            (unsigned long long)G, (unsigned long long)ntiles, (unsigned long long)t,
            (unsigned long long)(base + below), (unsigned long long)prefix[t]);
      CHECK(off == prefix[t], "G=%llu n=%llu tile %llu: carried offset %llu, prefix %llu",
            (unsigned long long)G, (unsigned long long)ntiles, (unsigned long long)t,
            (unsigned long long)off, (unsigned long long)prefix[t]);
      if (t == ntiles - 1) total = off + count[t];  // d_count[0]
    }
  }
  CHECK(total == prefix[ntiles], "G=%llu n=%llu: total %llu, prefix %llu", (unsigned long long)G,
        (unsigned long long)ntiles, (unsigned long long)total, (unsigned long long)prefix[ntiles]);
}

int main() {
  const u64 grids[] = {1, 2, 3, 7, 511, 512, 1023, 1024};
  for (u64 G : grids) {
    const u64 ge = (G + 1) / 2;
    // one stripe (full, and part of one); a full last stripe; a last stripe of E tiles
    // only (all of E, and one short of it); a last stripe of one tile
    const u64 shapes[] = {G, ge, 1, 3 * G, 2 * G + ge, 2 * G + (ge > 1 ? ge - 1 : ge), 2 * G + 1, 4 * G + 1};
    for (u64 n : shapes) run(G, n);
  }
  printf("%ld checks, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
