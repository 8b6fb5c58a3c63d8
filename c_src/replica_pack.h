/*
 * replica_pack.h — the replica layer's host layouts, each stated once: rows and a context as
 * columns at one stride, the packed messages, the return block, a continuation's byte frame.
 * Host code only (replica_pack.c calls no dg_* function); internal, not the NIF's surface.
 */
#ifndef DG_REPLICA_PACK_H
#define DG_REPLICA_PACK_H

#include "../include/deltagpu.h"

static inline uint64_t even(uint64_t w) { return (w + 1) & ~UINT64_C(1); } /* 16-B aligned offsets */
static inline uint64_t rows_words(uint64_t n) { return 4 * even(n) + even((n + 1) / 2); }
static inline uint64_t ctx_words(uint64_t n) { return even(n) + even((n + 1) / 2); }

/* Rows as five columns `stride` words apart: key | val | ts | cnt | node (u32) from `base`
 * (the column order; dg_store's fields name node before cnt). */
dg_store rp_rows(uint64_t* base, uint64_t stride, uint64_t n, uint64_t cap);
/* A context as two columns `stride` words apart: cnt | node (u32). */
dg_context rp_ctx(uint64_t* base, uint64_t stride, int32_t kind, uint64_t n, uint64_t cap);

/* host rows / a host context into the message `hb` at word o, columns at stride even(n);
 * *dev = the view of the same place in its device copy `db`.  Returns the next free word. */
uint64_t rp_pack_rows(uint64_t* hb, uint64_t* db, uint64_t o, const dg_store* r, dg_store* dev);
uint64_t rp_pack_ctx(uint64_t* hb, uint64_t* db, uint64_t o, const dg_context* c, dg_context* dev);
/* keys -> ascending unique at dst; returns their number */
uint64_t rp_sort_unique(const uint64_t* keys, uint64_t n, uint64_t* dst);
/* host rows in store order without duplicates / a context in its kind's order (O(n) walks) */
int rp_rows_sorted(const dg_store* s);
int rp_ctx_sorted(const dg_context* c);

/* The return block for S changed keys / rows and a context of C entries (words): changed
 * keys [0, S) | key | val | ts | cnt [S, 5S) | node u32 [5S, 6S) | context cnt [6S, 6S + C) |
 * context node u32 [6S + C, 6S + 2C) | the changed keys' old value ids [D, D + S) | new
 * [D + S, D + 2S) | flags u8 [D + 2S, D + 2S + S / 8], D = 6S + 2C (the *_diffs calls).  The
 * kernels write it and the term layers read these views of it (here empty: n = 0, a VV). */
static inline uint64_t rp_back_words(uint64_t S, uint64_t C) { return 6 * S + 2 * C + 2 * S + S / 8 + 1; }
static inline uint64_t* rp_back_keys(uint64_t* b) { return b; }
static inline dg_store rp_back_rows(uint64_t* b, uint64_t S) { return rp_rows(b + S, S, 0, S); }
static inline dg_context rp_back_ctx(uint64_t* b, uint64_t S, uint64_t C) {
  return rp_ctx(b + 6 * S, C, DG_CTX_VV, 0, C);
}
static inline dg_lww_diffs rp_back_diffs(uint64_t* b, uint64_t S, uint64_t C) {
  uint64_t* d = b + 6 * S + 2 * C;
  return (dg_lww_diffs){d, d + S, (uint8_t*)(d + 2 * S), S};
}
/* the least S with n bytes at the block's head, the 6 S words before the context (dgr_sweep) */
static inline uint64_t rp_back_s_for_bytes(uint64_t n) { return (n + 6 * 8 - 1) / (6 * 8); }

/* A continuation as bytes (replica.h dgr_merkle_prepare): a 20-byte header, then the words
 * pos[n] | hash[n] | bucket[n_buckets]. */
#define RP_CONT_HEAD 20
static inline uint64_t rp_cont_bytes(uint64_t n, uint64_t nb) { return RP_CONT_HEAD + 8 * (2 * n + nb); }
/* writes the header; returns where pos | hash | bucket go */
uint8_t* rp_cont_write_head(uint8_t* bin, uint32_t level, uint64_t n, uint64_t n_buckets);
/* the header of a frame of `len` bytes read and checked against len (DG_E_INVAL) */
int rp_cont_parse(const uint8_t* bin, uint64_t len, uint32_t* level, uint64_t* n, uint64_t* n_buckets);
/* the continuation whose pos | hash | bucket run stands at `base` (full: n = cap) */
dg_merkle_cont rp_cont_at(uint64_t* base, uint32_t level, uint64_t n, uint64_t n_buckets);


/* What one hop through dg_merkle_continue_home / dg_merkle_continues is given for its results,
 * in page-locked words: C entries (pos | hash) and CB buckets for the next continuation, kcap
 * keys.  From the incoming continuation (level, n entries) on a tree of `depth` over rows_n
 * rows: a node form above the buckets expands to at most n << k children, k = min(levels,
 * depth - level), truncated to max_sync; at the bucket level four pairs per bucket (at least
 * 64), grown once to what the call reports; the keys are the first max_sync, at most every
 * key of both sides and RP_CONT_SMALL_OUT.  A hop whose C exceeds RP_CONT_SMALL_OUT takes the
 * general path. */
#define RP_CONT_SMALL_OUT 65536 /* entries of an outgoing continuation / keys kept in host memory */
typedef struct rp_cont_room {
  uint64_t C, CB, kcap;
} rp_cont_room;
static inline uint64_t rp_u64min(uint64_t a, uint64_t b) { return a < b ? a : b; }
static inline uint64_t rp_u64max(uint64_t a, uint64_t b) { return a > b ? a : b; }
static inline rp_cont_room rp_cont_room_for(uint32_t level, uint64_t n, uint32_t depth, uint32_t levels,
                                            uint64_t max_sync, uint64_t rows_n) {
  rp_cont_room r;
  r.CB = rp_u64max(rp_u64min(n, max_sync), 1);
  if (level < depth) {
    const uint32_t k = levels < depth - level ? levels : depth - level;
    r.C = rp_u64min(n << k, max_sync);
  } else {
    r.C = rp_u64max(4 * rp_u64min(n, max_sync), 64);
  }
  r.C = rp_u64max(r.C, 1);
  r.kcap = rp_u64max(rp_u64min(rp_u64min(max_sync, rows_n + n + 1), RP_CONT_SMALL_OUT), 1);
  return r;
}
/* The k hops' rooms carved from ONE block, end to end: hop j's words are pos [off[j], +C) |
 * hash [+C, +2C) | bucket [+2C, +2C + CB) | keys [+2C + CB, +2C + CB + kcap), every region on
 * an 8-byte word and none shared.  Returns the block's words (off[k] is written too). */
static inline uint64_t rp_cont_carve(int k, const rp_cont_room* room, uint64_t* off) {
  uint64_t w = 0;
  for (int j = 0; j < k; j++) {
    off[j] = w;
    w += 2 * room[j].C + room[j].CB + room[j].kcap;
  }
  off[k] = w;
  return w;
}
/* hop j's output continuation (empty: n = 0) and keys inside the block at `base` */
static inline dg_merkle_cont rp_cont_room_out(uint64_t* base, uint64_t off, rp_cont_room r) {
  dg_merkle_cont c;
  c.level = 0;
  c.reserved = 0;
  c.pos = base + off;
  c.hash = base + off + r.C;
  c.n = 0;
  c.cap = r.C;
  c.bucket = base + off + 2 * r.C;
  c.n_buckets = 0;
  c.cap_buckets = r.CB;
  return c;
}
static inline uint64_t* rp_cont_room_keys(uint64_t* base, uint64_t off, rp_cont_room r) {
  return base + off + 2 * r.C + r.CB;
}

/* The row room of a hop that is answered with its rows (dg_merkle_continues_take), in page-locked
 * words: R rows as rp_rows lays them out (columns at stride even(R)), then kcap + 1 offsets.
 * dgr_take's "four rows per key" rule with a ceiling: R = min(rows_n, 4 * min(kcap, 4096) + 64),
 * about 31 KB per hop at max_sync_size 200.  A hop that needs more takes its rows through
 * dg_take_keysets afterwards. */
typedef struct rp_take_room {
  uint64_t R, kcap;
} rp_take_room;
static inline rp_take_room rp_take_room_for(uint64_t kcap, uint64_t rows_n) {
  rp_take_room r;
  r.R = rp_u64min(rows_n, 4 * rp_u64min(kcap, 4096) + 64);
  r.kcap = kcap;
  return r;
}
static inline uint64_t rp_take_room_words(rp_take_room r) { return rows_words(r.R) + even(r.kcap + 1); }
/* The k hops' row rooms carved from ONE block (another than rp_cont_carve's), end to end: hop j's
 * words are its rows [off[j], + rows_words(R)) | offsets [+ rows_words(R), + kcap + 1), each hop on
 * a 16-byte boundary and no word shared.  Returns the block's words (off[k] is written too). */
static inline uint64_t rp_take_carve(int k, const rp_take_room* room, uint64_t* off) {
  uint64_t w = 0;
  for (int j = 0; j < k; j++) {
    off[j] = w;
    w += rp_take_room_words(room[j]);
  }
  off[k] = w;
  return w;
}
static inline dg_store rp_take_room_rows(uint64_t* base, uint64_t off, rp_take_room r) {
  return rp_rows(base + off, even(r.R), 0, r.R);
}
static inline uint64_t* rp_take_room_offs(uint64_t* base, uint64_t off, rp_take_room r) {
  return base + off + rows_words(r.R);
}

#endif /* DG_REPLICA_PACK_H */
