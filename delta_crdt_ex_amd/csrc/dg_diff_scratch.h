// dg_diff_scratch.h — the full Merkle diff's tiling and the layout of its scratch, as plain
// arithmetic (no HIP: tests/diff_take_layout.cc builds it on the host).  merkle_diff.hip carves
// the words, api_merkle.hip sizes the engine's scratch by them.
#pragma once
#include <stdint.h>

namespace dg {

constexpr int DIFF_BLOCK = 256;
#ifndef DG_DIFF_SUB
#define DG_DIFF_SUB 12
#endif
constexpr uint32_t DIFF_SUB = DG_DIFF_SUB;  // levels a diff workgroup descends: subtrees of 2^DIFF_SUB buckets
inline uint32_t diff_sub(uint32_t depth) { return depth < DIFF_SUB ? depth : DIFF_SUB; }
inline uint64_t diff_tiles(uint32_t depth) { return 1ull << (depth - diff_sub(depth)); }
// subtree boundaries in both stores, per-subtree counts, then the differing keys staged
// per subtree (at most one per row of either store), then the group sums
inline uint64_t diff_groups(uint32_t depth) { return (diff_tiles(depth) + DIFF_BLOCK - 1) / DIFF_BLOCK; }  // of DIFF_BLOCK subtrees
inline uint64_t diff_scratch_words(uint32_t depth, uint64_t na, uint64_t nb) {
  return 2 * (diff_tiles(depth) + 1) + diff_tiles(depth) + na + nb + 1;
}

// dg_merkle_diff_take's scratch: dg_merkle_diff's words in their places (bnd, cnt, keys), then
// one located word per possible differing key, beside keys[x], and the per-subtree row counts.
// It grows by na + nb + 1 + diff_tiles words over the diff's, for the take form only.
struct DiffTakeScratch {
  uint64_t bnd, cnt, keys, loc, rcnt, words;  // word offsets of the arrays, and the size of the whole
};
inline DiffTakeScratch diff_take_scratch(uint32_t depth, uint64_t na, uint64_t nb) {
  const uint64_t nt = diff_tiles(depth);
  DiffTakeScratch s;
  s.bnd = 0;                  // 2 x (nt + 1) subtree boundaries
  s.cnt = 2 * (nt + 1);       // nt key counts
  s.keys = s.cnt + nt;        // na + nb keys (+ 1)
  s.loc = diff_scratch_words(depth, na, nb);  // na + nb located runs (+ 1)
  s.rcnt = s.loc + na + nb + 1;               // nt row counts
  s.words = s.rcnt + nt;
  return s;
}
inline uint64_t diff_take_scratch_words(uint32_t depth, uint64_t na, uint64_t nb) {
  return diff_take_scratch(depth, na, nb).words;
}

}  // namespace dg
