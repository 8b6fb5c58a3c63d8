/*
 * replica_int.h — what the replica layer's files (replica.c and replica_join.c,
 * replica_take.c, replica_merkle.c: one per call family) share: the engine, the state and
 * the engine's buffer helpers (replica.c).  Internal: not the NIF's surface.
 */
#ifndef DG_REPLICA_INT_H
#define DG_REPLICA_INT_H

#include <stdlib.h>
#include <string.h>

#include "replica.h"
#include "replica_pack.h"

struct dgr_state {
  dgr_engine* g;
  dg_store rows;
  dg_store spare; /* dg_join_delta's second buffer (allocated on first need, kept) */
  dg_context ctx;
  dg_merkle tree;
  int has_tree;
  uint64_t version;
  dgr_state *prev, *next;
};

struct dgr_engine {
  dg_engine* e;
  dgr_state* live;
  uint64_t n_live;
  /* the universe's term hashes on the device; every tree points at th */
  dg_term_hashes th;
  uint64_t *d_nh, *d_vid, *d_vh;
  uint64_t nh_cap, vid_cap, vh_cap;
  uint64_t th_nodes, th_vals;
  int th_stale;
  /* the packed message (a delta, a key list, ops, a continuation): page-locked host
   * words and their device copy */
  uint64_t *h_msg, *d_msg;
  uint64_t msg_cap;
  /* a delta sorted on the device when the map walk did not give the order */
  dg_store drows;
  dg_context dctx;
  /* a batch of deltas (dgr_join_deltas): the device views of each delta's rows, context
   * and keyset inside the message (or inside drows / dctx, once sorted); ONE allocation */
  dg_store* b_rows;
  dg_context* b_ctx;
  const uint64_t** b_keys;
  uint64_t* b_nk;
  uint8_t* b_unsorted; /* bit 0: the rows, bit 1: the context */
  uint64_t b_cap;
  /* dg_mutate_batch's delta, its dot list and touched keys */
  dg_store mrows;
  dg_context mctx;
  uint64_t* mkeys;
  uint64_t mkeys_cap;
  /* the return block (replica_pack.h rp_back_*) for back_s keys / rows, back_c context entries */
  uint64_t *d_back, *h_back;
  uint64_t back_s, back_c;
  /* dg_join_delta_home's result block (page-locked, DG_HOME_DIFFS_WORDS: the plain call
   * writes a prefix of it) */
  uint64_t* h_home;
  /* read output: keys [0, cap) | values [cap, 2 cap) */
  uint64_t *d_rd, *h_rd;
  uint64_t rd_cap, h_rd_cap;
  /* take output */
  dg_store tk;
  uint64_t* h_tk;
  uint64_t h_tk_cap;
  /* dgr_take_batch: union keys [0, K) | masks [K, 2K) | offsets [2K, 3K + 1), K = tb_cap */
  uint64_t *d_tb, *h_tb;
  uint64_t tb_cap;
  /* continuations: the output (device), the keys, and the bytes handed back */
  dg_merkle_cont co;
  uint64_t *d_ckeys, *h_ckeys, *h_cstage;
  uint64_t ckeys_cap, h_ckeys_cap, h_cstage_cap;
  uint8_t* h_bin;
  uint64_t bin_cap;
  /* dgr_merkle_continue_batch: the k hops' outputs (page-locked, replica_pack.h rp_cont_carve) */
  uint64_t* h_bstage;
  uint64_t h_bstage_cap;
  /* dgr_merkle_continue_take_batch: the hops' rows and offsets out of the launch (page-locked,
   * rp_take_carve), and those of the hops that took theirs through dgr_take_batch, per hop */
  uint64_t *h_tstage, *h_tfall;
  uint64_t h_tstage_cap, h_tfall_cap;
  /* dgr_sync_from: the kept keys and their row offsets (device: keys [0, cap) | offs behind
   * them), and the source's rows of those keys */
  uint64_t* d_sy;
  uint64_t sy_cap;
  dg_store sy_rows;
  /* dgr_sweep: the live states' stores as one host array */
  dg_store* sw_stores;
  uint64_t sw_cap;
  /* dgr_join_deltas' route (DGR_DELTAS_ROUTE=stream|keyed|auto, read at engine open), and how
   * often it tried dg_join_deltas_keyed, was served and was declined (dgr_deltas_route_stats) */
  int deltas_route;
  uint64_t keyed_stats[3];
  /* dgr_mutate_batch's route (DGR_MUTATE_ROUTE=batch|home, read at engine open), and how often
   * it tried dg_mutate_home, was served and was declined (dgr_mutate_route_stats) */
  int mutate_route;
  uint64_t mutate_stats[3];
};

enum { DGR_ROUTE_AUTO = 0, DGR_ROUTE_STREAM = 1, DGR_ROUTE_KEYED = 2 };
enum { DGR_MROUTE_BATCH = 0, DGR_MROUTE_HOME = 1 };

#define TRY(x)                     \
  do {                             \
    const int rc_ = (x);           \
    if (rc_ != DG_OK) return rc_;  \
  } while (0)

static inline uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }
static inline uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }

static inline int check_version(const dgr_state* s, uint64_t version) {
  return version == s->version ? DG_OK : DGR_E_STALE;
}

/* The engine's buffers (replica.c), grown on demand, contents not kept.  ri_renew is the one
 * free-and-allocate: *h (page-locked host) and / or *d (device; NULL: absent) at `words` words
 * each, *cap = `want` once they stand and 0 until then.  ri_grow: ONE buffer, host or device;
 * it doubles and adds 16, as stores and contexts do. */
int ri_renew(dgr_engine* g, uint64_t** h, uint64_t** d, uint64_t* cap, uint64_t want, uint64_t words);
int ri_grow(dgr_engine* g, uint64_t** h, uint64_t** d, uint64_t* cap, uint64_t words);
int ri_grow_msg(dgr_engine* g, uint64_t words); /* host and device; doubles and adds 64 */
int ri_grow_store(dgr_engine* g, dg_store* s, uint64_t n);
int ri_grow_ctx(dgr_engine* g, dg_context* c, uint64_t n);
int ri_grow_back(dgr_engine* g, uint64_t S, uint64_t C); /* the return block */
int ri_grow_batch(dgr_engine* g, uint64_t k);            /* the b_* arrays */
void ri_free_tree(dgr_state* s);
/* dgr_take / dgr_take_batch behind their argument and version checks (replica_take.c) */
int ri_take(dgr_state* s, const uint64_t* keys, uint64_t n_keys, dg_store* out);
int ri_take_batch(dgr_state* s, int k, const uint64_t* const* keys, const uint64_t* n_keys, dgr_taken* out);

#endif /* DG_REPLICA_INT_H */
