// dg_arena.h — the scratch layouts of the C-ABI layer, each written once.  Host only, no
// HIP: a layout function takes an Arena and the sizes it needs and returns the pointers.
// The caller runs it on a measuring arena (null base) for the byte count, grows the buffer,
// and runs it again on the buffer: the size and the pointers come from the same lines
// (tests/arena_layouts.cc checks every layout against its offsets and under ASan).
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/deltagpu.h"

namespace dg {

constexpr size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A bump allocator over a buffer that need not exist yet.  Regions start where the one
// before ended; `align` rounds a region's SIZE (256 B: every region of a 256-B aligned
// buffer then starts 256-B aligned, and a column of an odd row count has padding behind
// it, which the 16-byte pair stores of the splice and the one-wait join rely on).
struct Arena {
  char* base;
  size_t off = 0;
  explicit Arena(void* b = nullptr) : base((char*)b) {}
  template <class T>
  T* take(size_t count, size_t align = 256) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += round_up(count * sizeof(T), align);
    return p;
  }
  void align_to(size_t a) { off = round_up(off, a); }
  // A store of `rows` rows (n = 0); the column order is part of the layout.
  dg_store store(uint64_t rows) {
    dg_store s{};
    s.key = take<uint64_t>(rows);
    s.val = take<uint64_t>(rows);
    s.ts = take<int64_t>(rows);
    s.cnt = take<uint64_t>(rows);
    s.node = take<uint32_t>(rows);
    s.cap = rows;
    return s;
  }
  // A context of `cap` entries (n = 0, a version vector until a join says otherwise).
  dg_context context(uint64_t cap) {
    dg_context c{};
    c.cnt = take<uint64_t>(cap);
    c.node = take<uint32_t>(cap);
    c.cap = cap;
    c.kind = DG_CTX_VV;
    return c;
  }
  // the buffer to allocate: never empty, so that no carved pointer is null
  size_t bytes() const { return off ? round_up(off, 256) : 256; }
};

// join2_enqueue (engine tmp): the context union's scratch | the two-pass join's counts
// (pass_bytes 0: single pass) | the change events (chg_bytes 0: none, chg null)
struct JoinScratch {
  void *ctx, *pass, *chg;
};
inline JoinScratch join_layout(Arena& a, size_t ctx_bytes, size_t pass_bytes, size_t chg_bytes) {
  JoinScratch s;
  s.ctx = a.take<char>(ctx_bytes);
  s.pass = a.take<char>(pass_bytes);
  s.chg = chg_bytes ? a.take<char>(chg_bytes) : nullptr;
  return s;
}

// The bytes a layout asks for: what its caller passes on as a region of another layout.
template <class Layout>
size_t measured(Layout layout) {
  Arena m;
  layout(m);
  return m.bytes();
}

// The three scratch layouts below are carved by the join's launchers (join*.hip) and
// measured by join2_enqueue; `tile` is JOIN_TILE (this header knows no kernel constant).

// The join's share of the engine's u64 state words (Scan::state; sized for the tiles after
// a re-cut, join2_tiles_cap, carved for the tiles in use): ntiles words no join kernel
// touches (the look-back granules of the kernel before the stripe counts; they keep the
// splits where they were) | the merge-path split of every tile boundary (ntiles + 1) | the
// keyset splits (ntiles + 1)
struct JoinState {
  uint64_t *splits, *ksplits;
};
inline JoinState join_state_layout(Arena& a, uint64_t ntiles) {
  JoinState s;
  a.take<uint64_t>(ntiles, 8);
  s.splits = a.take<uint64_t>(ntiles + 1, 8);
  s.ksplits = a.take<uint64_t>(ntiles + 1, 8);
  return s;
}

// The two-pass join (join_layout's pass): kept rows per tile | per tile its compaction
// list, `tile` u16 LDS slot numbers
struct PassScratch {
  uint32_t* counts;
  unsigned short* lists;
};
inline PassScratch pass_layout(Arena& a, uint64_t ntiles, uint64_t tile) {
  PassScratch s;
  s.counts = a.take<uint32_t>(ntiles);
  s.lists = a.take<unsigned short>(ntiles * tile);
  return s;
}

// The change events (join_layout's chg): per tile `tile` event keys | the chunk summaries
// (ntiles x 8 bytes) | per tile its event count, its events that differ from their
// predecessor, and a third u32 nothing uses (it keeps the offsets behind it) | per tile
// its first and its last event.  A chunk summary (join_changes.hip ChgSum) covers
// CHG_CHUNK tiles; the last chunk's is never written, so ceil(ntiles / CHG_CHUNK) - 1 of
// them must fit their region.
constexpr uint64_t CHG_CHUNK = 64;
constexpr size_t CHG_SUM_BYTES = 32;
struct ChgScratch {
  uint64_t* ev;
  void* chunk;
  uint32_t *cnt, *wu;
  uint64_t *fk, *lk;
};
inline ChgScratch chg_layout(Arena& a, uint64_t ntiles, uint64_t tile) {
  ChgScratch s;
  s.ev = a.take<uint64_t>(ntiles * tile, 8);
  s.chunk = a.take<char>(ntiles * 8, 8);
  const uint64_t chunks = (ntiles + CHG_CHUNK - 1) / CHG_CHUNK;
  assert(chunks <= 1 || (chunks - 1) * CHG_SUM_BYTES <= ntiles * 8);
  (void)chunks;
  s.cnt = a.take<uint32_t>(ntiles, 4);
  s.wu = a.take<uint32_t>(ntiles, 4);
  a.take<uint32_t>(ntiles, 4);
  a.align_to(8);
  s.fk = a.take<uint64_t>(ntiles, 8);
  s.lk = a.take<uint64_t>(ntiles, 8);
  return s;
}

// The per-key index of a splice: five arrays of nk + 1 entries
struct KeyIndex {
  uint64_t *a_lo, *a_off, *end;
  int64_t *shift, *gap;
};
inline KeyIndex key_index(Arena& a, uint64_t nk) {
  KeyIndex x;
  x.a_lo = a.take<uint64_t>(nk + 1);
  x.a_off = a.take<uint64_t>(nk + 1);
  x.end = a.take<uint64_t>(nk + 1);
  x.shift = a.take<int64_t>(nk + 1);
  x.gap = a.take<int64_t>(nk + 1);
  return x;
}

// The splice (engine spl): the state's rows of the keyset | the edit | the per-key index |
// the per-tile entry ranges | the join's union context
struct SpliceScratch {
  dg_store ak, ed;
  KeyIndex idx;
  uint64_t* tile_u0;
  dg_context uctx;
};
inline SpliceScratch splice_layout(Arena& a, uint64_t cap_k, uint64_t cap_e, uint64_t nk, uint64_t a_tiles,
                                   uint64_t uctx_cap) {
  SpliceScratch s;
  s.ak = a.store(cap_k);
  s.ed = a.store(cap_e);
  s.idx = key_index(a, nk);
  s.tile_u0 = a.take<uint64_t>(a_tiles + 1);
  s.uctx = a.context(uctx_cap);
  return s;
}

// dg_join_delta's one-wait path (engine kdb): seven per-key figures | shift (nk + 1) | the
// count workgroups' figures | the per-tile entry ranges | the union context and its
// scratch | with diffs, the per-key winners (last, and only then)
struct KdScratch {
  uint64_t *a_lo, *d_lo, *runs, *amask, *dmask, *dh, *end;
  int64_t* shift;
  uint64_t *part, *tile_u0;
  dg_context uctx;
  void* cu_tmp;
  uint64_t *dv_old, *dv_new;
};
inline KdScratch kd_layout(Arena& a, uint64_t nk, uint64_t part_words, uint64_t a_tiles, uint64_t uctx_cap,
                           size_t cu_bytes, bool diffs) {
  KdScratch s;
  for (uint64_t** q : {&s.a_lo, &s.d_lo, &s.runs, &s.amask, &s.dmask, &s.dh, &s.end}) *q = a.take<uint64_t>(nk);
  s.shift = a.take<int64_t>(nk + 1);
  s.part = a.take<uint64_t>(part_words);
  s.tile_u0 = a.take<uint64_t>(a_tiles + 2);
  s.uctx = a.context(uctx_cap);
  s.cu_tmp = a.take<char>(cu_bytes);
  s.dv_old = diffs ? a.take<uint64_t>(nk) : nullptr;
  s.dv_new = diffs ? a.take<uint64_t>(nk) : nullptr;
  return s;
}

// dg_join_delta_home (engine sml): the edit | the per-key index | a sixth array of its size:
// dg_mutate_home's touched keys (nk = its ops: at most as many keys), which the kernel
// writes and the splice after the wait reads; the join has its keyset from the caller and
// leaves it unused | the per-tile entry ranges | the moved word | the result block
struct HomeScratch {
  dg_store ed;
  KeyIndex idx;
  uint64_t* keys;
  uint64_t* tile_u0;
  uint32_t* moved;
  uint64_t* res;
};
inline HomeScratch home_layout(Arena& a, uint64_t edit_rows, uint64_t nk, uint64_t a_tiles,
                               uint64_t result_words) {
  HomeScratch s;
  s.ed = a.store(edit_rows);
  s.idx = key_index(a, nk);
  s.keys = a.take<uint64_t>(nk + 1);
  s.tile_u0 = a.take<uint64_t>(a_tiles + 2);
  s.moved = a.take<uint32_t>(1);
  s.res = a.take<uint64_t>(result_words);
  return s;
}

// The tree update's scratch: the hand-off words | the dirty flags (u32, padded to even so
// that cdelta is 8-byte aligned) | the per-chunk row-count changes.  dg_merkle_update has
// all three in engine tmp (hand and flags the same arena); the one-wait path keeps the
// flags and changes in a buffer of their own that stays zero between calls.  zero_words:
// the u32 words from `dirty` on, which one launch zeroes.
struct TreeScratch {
  uint64_t* hand;
  uint32_t* dirty;
  int64_t* cdelta;
  uint64_t zero_words;
};
inline TreeScratch tree_layout(Arena& hand, Arena& flags, uint64_t ctr_words, uint64_t chunks) {
  const uint64_t cpad = (chunks + 1) & ~1ull;
  TreeScratch s;
  s.hand = (uint64_t*)hand.take<uint32_t>(ctr_words, 8);
  s.dirty = flags.take<uint32_t>(cpad, 8);
  s.cdelta = flags.take<int64_t>(chunks, 8);
  s.zero_words = cpad + 2 * chunks;
  return s;
}

// A fold's two intermediate states (engine fold).  The one PACKED layout: columns are not
// padded, so a column's alignment -- and with it whether a stepwise fold's intermediate
// passes pair_aligned and splices -- follows the parity of `rows`.  Each half ends with 1 KiB
// of padding, rounded up to 256 B.
struct FoldScratch {
  dg_store st[2];
  dg_context cx[2];
};
inline FoldScratch fold_layout(Arena& a, uint64_t rows, uint64_t ctx) {
  FoldScratch s;
  for (int w = 0; w < 2; w++) {
    dg_store& st = s.st[w] = dg_store{};
    dg_context& cx = s.cx[w] = dg_context{};
    st.key = a.take<uint64_t>(rows, 8);
    st.val = a.take<uint64_t>(rows, 8);
    st.ts = a.take<int64_t>(rows, 8);
    st.cnt = a.take<uint64_t>(rows, 8);
    cx.cnt = a.take<uint64_t>(ctx, 8);
    st.node = a.take<uint32_t>(rows, 4);
    cx.node = a.take<uint32_t>(ctx, 4);
    a.take<char>(1024, 1);
    a.align_to(256);
    st.cap = rows;
    cx.cap = ctx;
    cx.kind = DG_CTX_VV;
  }
  return s;
}

// The one-pass fold (kfold_pass).  Staged in pinned memory and copied to the head of engine
// tmp: the k run descriptors | the dots' offsets (k + 1).  Behind them on the device: the
// state's bucket starts (T + 1) | the deltas' (T + 1 per run and kind) | the two VV tables
// (k * nodes each) | the flag | the dot set (dset_n 0: no DOTS delta, dset null).
struct KfoldStaged {
  void* runs;
  uint64_t* cflat;
};
inline KfoldStaged kfold_staged_layout(Arena& a, uint64_t k, size_t run_bytes) {
  KfoldStaged s;
  s.runs = a.take<char>(k * run_bytes);
  s.cflat = a.take<uint64_t>(k + 1);
  return s;
}
struct KfoldScratch {
  KfoldStaged staged;
  size_t staged_bytes;  // what the host copies in
  uint64_t* sstart;
  uint32_t* dstart;
  uint64_t *tabC, *tabP;
  uint32_t* flag;
  size_t zero_bytes;  // from sstart through the flag: zeroed per attempt
  uint64_t* dset;
};
inline KfoldScratch kfold_layout(Arena& a, uint64_t k, size_t run_bytes, uint64_t T, uint64_t nodes,
                                 uint64_t dset_n) {
  KfoldScratch s;
  s.staged = kfold_staged_layout(a, k, run_bytes);
  s.staged_bytes = a.off;
  s.sstart = a.take<uint64_t>(T + 1);
  s.dstart = a.take<uint32_t>((T + 1) * 2 * k);
  s.tabC = a.take<uint64_t>(k * nodes);
  s.tabP = a.take<uint64_t>(k * nodes);
  s.flag = a.take<uint32_t>(1);
  s.zero_bytes = a.off - s.staged_bytes;
  s.dset = dset_n ? a.take<uint64_t>(dset_n) : nullptr;
  return s;
}

// The streaming store diff (engine tmp): the diagonals' bounds (4 per diagonal, tiles + 1
// diagonals) | per tile the changed keys, their rows and the two offsets | the changed mask
// (u32 words, zeroed per call)
struct SdiffScratch {
  uint64_t* bounds;
  uint64_t *cnt_k, *cnt_r, *off_k, *off_r;
  uint32_t* mask;
};
inline SdiffScratch sdiff_layout(Arena& a, uint64_t tiles, uint64_t mask_words) {
  SdiffScratch s;
  s.bounds = a.take<uint64_t>(4 * (tiles + 1));
  for (uint64_t** q : {&s.cnt_k, &s.cnt_r, &s.off_k, &s.off_r}) *q = a.take<uint64_t>(tiles);
  s.mask = a.take<uint32_t>(mask_words);
  return s;
}

// dg_mutate_batch (engine tmp): the delta's dots (node | cnt) | their sort's second pair |
// the sort's scratch
struct MutateScratch {
  uint32_t* dnode;
  uint64_t* dcnt;
  uint32_t* tnode;
  uint64_t* tcnt;
  void* sort_tmp;
};
inline MutateScratch mutate_layout(Arena& a, uint64_t n_dots, size_t sort_bytes) {
  MutateScratch s;
  s.dnode = a.take<uint32_t>(n_dots);
  s.dcnt = a.take<uint64_t>(n_dots);
  s.tnode = a.take<uint32_t>(n_dots);
  s.tcnt = a.take<uint64_t>(n_dots);
  s.sort_tmp = a.take<char>(sort_bytes);
  return s;
}

// dg_mark_ids (engine tmp): the column descriptors (n_stores + 1, staged in pinned memory
// first) | the bitmap | the id samples
struct MarkScratch {
  void* segs;
  uint32_t* bitmap;
  uint64_t* samples;
};
inline MarkScratch mark_layout(Arena& a, uint64_t n_stores, size_t seg_bytes, uint64_t bitmap_words,
                               uint64_t samples) {
  MarkScratch s;
  s.segs = a.take<char>((n_stores + 1) * seg_bytes);
  s.bitmap = a.take<uint32_t>(bitmap_words);
  s.samples = a.take<uint64_t>(samples);
  return s;
}

// dg_take_keysets (engine tmp): the keyset descriptors (k + 1, staged in pinned memory first)
// | the m items end to end and their set numbers | the union keys | the take's per-key
// first rows and offsets (m + 1) | the sort's scratch
struct TakesetsScratch {
  void* segs;
  uint64_t* cat;
  uint8_t* set;
  uint64_t *ukeys, *key_lo, *key_off;
  void* sort_tmp;
};
inline TakesetsScratch takesets_layout(Arena& a, uint64_t k, size_t seg_bytes, uint64_t m, size_t sort_bytes) {
  TakesetsScratch s;
  s.segs = a.take<char>((k + 1) * seg_bytes);
  s.cat = a.take<uint64_t>(m);
  s.set = a.take<uint8_t>(m);
  s.ukeys = a.take<uint64_t>(m);
  s.key_lo = a.take<uint64_t>(m);
  s.key_off = a.take<uint64_t>(m + 1);
  s.sort_tmp = a.take<char>(sort_bytes);
  return s;
}

// dg_join_deltas_keyed (engine kdb).  The union's part is dg_take_keysets': the keyset
// descriptors (k + 1) and the run descriptors (k), both staged in pinned memory first | the m
// items end to end and their set numbers | the union in sorted order | the sort's scratch.
// Behind it what outlives the union: the union keys and masks (m) | the two VV tables
// (k * nodes each), the flag and the edit store's bump pointer -- zero_bytes from tabC on,
// zeroed per call | the edit store (e_rows) | the one-wait path's own layout for m keys
// (kd_layout: the union has at most m keys).
struct KeyedScratch {
  void *segs, *runs;
  uint64_t* cat;
  uint8_t* set;
  uint64_t* usorted;
  void* sort_tmp;
  uint64_t *ukeys, *masks;
  uint64_t *tabC, *tabP;
  uint32_t* flag;
  uint64_t* e_next;
  size_t zero_bytes;
  dg_store ed;
  KdScratch kd;
};
inline KeyedScratch keyed_layout(Arena& a, uint64_t k, size_t seg_bytes, size_t run_bytes, uint64_t m,
                                 size_t sort_bytes, uint64_t nodes, uint64_t e_rows, uint64_t part_words,
                                 uint64_t a_tiles, uint64_t uctx_cap, bool diffs) {
  KeyedScratch s;
  s.segs = a.take<char>((k + 1) * seg_bytes);
  s.runs = a.take<char>(k * run_bytes);
  s.cat = a.take<uint64_t>(m);
  s.set = a.take<uint8_t>(m);
  s.usorted = a.take<uint64_t>(m);
  s.sort_tmp = a.take<char>(sort_bytes);
  s.ukeys = a.take<uint64_t>(m);
  s.masks = a.take<uint64_t>(m);
  const size_t z0 = a.off;
  s.tabC = a.take<uint64_t>(k * nodes);
  s.tabP = a.take<uint64_t>(k * nodes);
  s.flag = a.take<uint32_t>(1);
  s.e_next = a.take<uint64_t>(1);
  s.zero_bytes = a.off - z0;
  s.ed = a.store(e_rows);
  s.kd = kd_layout(a, m, part_words, a_tiles, uctx_cap, 0, diffs);
  return s;
}

// dg_replace_keysets (engine rpl; the splice behind it carves engine spl by splice_layout).
// Per item of the m keys laid end to end: its first row in its record's segment and its rows |
// per union key (at most m): the key, the winning record's first row and rows, the edit
// offsets (m + 1: the take's last tile writes entry n_keys) | per union tile its tails and
// their offset | the sort's scratch
struct ReplayScratch {
  uint64_t* item_lo;
  uint32_t* item_len;
  uint64_t *ukeys, *u_lo;
  uint32_t* u_len;
  uint64_t* e_off;
  uint64_t *tile_cnt, *tile_off;
  void* sort_tmp;
};
inline ReplayScratch replay_layout(Arena& a, uint64_t m, uint64_t union_tiles, size_t sort_bytes) {
  ReplayScratch s;
  s.item_lo = a.take<uint64_t>(m);
  s.item_len = a.take<uint32_t>(m);
  s.ukeys = a.take<uint64_t>(m);
  s.u_lo = a.take<uint64_t>(m);
  s.u_len = a.take<uint32_t>(m);
  s.e_off = a.take<uint64_t>(m + 1);
  s.tile_cnt = a.take<uint64_t>(union_tiles);
  s.tile_off = a.take<uint64_t>(union_tiles);
  s.sort_tmp = a.take<char>(sort_bytes);
  return s;
}

}  // namespace dg
