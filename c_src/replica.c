/*
 * replica.c — the NIF's device-resident replica state (replica.h): the engine and its buffers,
 * the term tables, relabels and sweeps, loading and freeing a state (the calls on a state:
 * replica_join.c, replica_take.c, replica_merkle.c; the host layouts: replica_pack.c).
 * Plain C over libdeltagpu's C-ABI (include/deltagpu.h); no term in sight.
 */
#include "replica_int.h"

/* ------------------------------------------------------------ buffers */
int ri_renew(dgr_engine* g, uint64_t** h, uint64_t** d, uint64_t* cap, uint64_t want, uint64_t words) {
  *cap = 0;
  if (h) TRY(dg_host_free(g->e, *h));
  if (d) TRY(dg_buffer_free(g->e, *d));
  if (h) *h = NULL;
  if (d) *d = NULL;
  if (h) TRY(dg_host_alloc(g->e, words * 8, (void**)h));
  if (d) TRY(dg_buffer_alloc(g->e, words * 8, (void**)d));
  *cap = want;
  return DG_OK;
}

int ri_grow(dgr_engine* g, uint64_t** h, uint64_t** d, uint64_t* cap, uint64_t words) {
  if (*(h ? h : d) && *cap >= words) return DG_OK;
  const uint64_t want = umax(words, 2 * *cap) + 16;
  return ri_renew(g, h, d, cap, want, want);
}

int ri_grow_msg(dgr_engine* g, uint64_t words) {
  if (g->h_msg && g->msg_cap >= words) return DG_OK;
  const uint64_t want = umax(words, 2 * g->msg_cap) + 64;
  return ri_renew(g, &g->h_msg, &g->d_msg, &g->msg_cap, want, want);
}

int ri_grow_store(dgr_engine* g, dg_store* s, uint64_t n) {
  if (s->key && s->cap >= n) return DG_OK;
  const uint64_t want = umax(n, 2 * s->cap) + 16;
  TRY(dg_store_free(g->e, s));
  return dg_store_alloc(g->e, want, s);
}

int ri_grow_ctx(dgr_engine* g, dg_context* c, uint64_t n) {
  if (c->node && c->cap >= n) return DG_OK;
  const int32_t kind = c->kind;
  TRY(dg_context_free(g->e, c));
  TRY(dg_context_alloc(g->e, umax(n, 2 * c->cap) + 16, c));
  c->kind = kind;
  return DG_OK;
}

/* for S changed keys / rows and a context of C entries: to the largest asked so far, no doubling */
int ri_grow_back(dgr_engine* g, uint64_t S, uint64_t C) {
  if (g->d_back && g->back_s >= S && g->back_c >= C) return DG_OK;
  S = umax(umax(S, g->back_s), 64);
  C = umax(umax(C, g->back_c), 64);
  TRY(ri_renew(g, &g->h_back, &g->d_back, &g->back_s, S, rp_back_words(S, C)));
  g->back_c = C;
  return DG_OK;
}

int ri_grow_batch(dgr_engine* g, uint64_t k) {
  if (g->b_cap >= k) return DG_OK;
  const uint64_t want = umax(k, 2 * g->b_cap) + 4;
  void* p = realloc(g->b_rows, want * (sizeof *g->b_rows + sizeof *g->b_ctx + sizeof *g->b_keys + 8 + 1));
  if (!p) return DG_E_NOMEM;
  g->b_rows = (dg_store*)p;
  g->b_ctx = (dg_context*)(g->b_rows + want);
  g->b_keys = (const uint64_t**)(g->b_ctx + want);
  g->b_nk = (uint64_t*)(g->b_keys + want);
  g->b_unsorted = (uint8_t*)(g->b_nk + want);
  g->b_cap = want;
  return DG_OK;
}

/* ------------------------------------------------------------ engine */
int dgr_deltas_route_stats(const dgr_engine* g, uint64_t out[3]) {
  if (!g || !out) return DG_E_INVAL;
  memcpy(out, g->keyed_stats, sizeof g->keyed_stats);
  return DG_OK;
}

int dgr_mutate_route_stats(const dgr_engine* g, uint64_t out[3]) {
  if (!g || !out) return DG_E_INVAL;
  memcpy(out, g->mutate_stats, sizeof g->mutate_stats);
  return DG_OK;
}

int dgr_engine_open(int device, dgr_engine** out) {
  if (!out) return DG_E_INVAL;
  *out = NULL;
  dgr_engine* g = (dgr_engine*)calloc(1, sizeof *g);
  if (!g) return DG_E_NOMEM;
  const int rc = dg_engine_create(device, NULL, &g->e);
  if (rc) {
    free(g);
    return rc;
  }
  g->th_stale = 1;
  g->mctx.kind = DG_CTX_DOTS;
  const char* route = getenv("DGR_DELTAS_ROUTE"); /* (tests and A/B: force dgr_join_deltas' route) */
  if (route && strcmp(route, "keyed") == 0) g->deltas_route = DGR_ROUTE_KEYED;
  if (route && strcmp(route, "stream") == 0) g->deltas_route = DGR_ROUTE_STREAM;
  /* dgr_mutate_batch's route: home unless told otherwise (faster on every shape measured: DESIGN 4.19) */
  route = getenv("DGR_MUTATE_ROUTE");
  g->mutate_route = DGR_MROUTE_HOME;
  if (route && strcmp(route, "batch") == 0) g->mutate_route = DGR_MROUTE_BATCH;
  *out = g;
  return DG_OK;
}

int dgr_engine_close(dgr_engine* g) {
  if (!g) return DG_OK;
  if (g->live) return DG_E_INVAL; /* states first */
  dg_engine* e = g->e;
  dg_buffer_free(e, g->d_nh);
  dg_buffer_free(e, g->d_vid);
  dg_buffer_free(e, g->d_vh);
  dg_host_free(e, g->h_msg);
  dg_buffer_free(e, g->d_msg);
  dg_store_free(e, &g->drows);
  dg_context_free(e, &g->dctx);
  dg_store_free(e, &g->mrows);
  dg_context_free(e, &g->mctx);
  dg_buffer_free(e, g->mkeys);
  dg_buffer_free(e, g->d_back);
  dg_host_free(e, g->h_back);
  dg_host_free(e, g->h_home);
  dg_buffer_free(e, g->d_rd);
  dg_host_free(e, g->h_rd);
  dg_store_free(e, &g->tk);
  dg_host_free(e, g->h_tk);
  dg_buffer_free(e, g->d_tb);
  dg_host_free(e, g->h_tb);
  dg_buffer_free(e, g->co.pos);
  dg_buffer_free(e, g->co.hash);
  dg_buffer_free(e, g->co.bucket);
  dg_buffer_free(e, g->d_ckeys);
  dg_host_free(e, g->h_ckeys);
  dg_host_free(e, g->h_cstage);
  dg_host_free(e, g->h_bstage);
  dg_host_free(e, g->h_tstage);
  dg_host_free(e, g->h_tfall);
  dg_buffer_free(e, g->d_sy);
  dg_store_free(e, &g->sy_rows);
  free(g->h_bin);
  free(g->sw_stores);
  free(g->b_rows); /* (and b_ctx, b_keys, b_nk, b_unsorted behind it) */
  const int rc = dg_engine_destroy(e);
  free(g);
  return rc;
}

dg_engine* dgr_dg(dgr_engine* g) { return g ? g->e : NULL; }
uint64_t dgr_live_states(const dgr_engine* g) { return g ? g->n_live : 0; }

int dgr_refresh_terms(dgr_engine* g, const uint64_t* node_hash, uint64_t n_nodes, const uint64_t* val_id,
                      const uint64_t* val_hash, uint64_t n_vals) {
  if (!g || (n_nodes && !node_hash) || (n_vals && (!val_id || !val_hash))) return DG_E_INVAL;
  if (g->th_stale || n_nodes != g->th_nodes) {
    g->th_nodes = 0;
    TRY(ri_grow(g, NULL, &g->d_nh, &g->nh_cap, n_nodes));
    TRY(dg_copy_to_device(g->e, g->d_nh, node_hash, n_nodes * 8));
    g->th_nodes = n_nodes;
  }
  if (g->th_stale || n_vals != g->th_vals) {
    g->th_vals = 0;
    TRY(ri_grow(g, NULL, &g->d_vid, &g->vid_cap, n_vals));
    TRY(ri_grow(g, NULL, &g->d_vh, &g->vh_cap, n_vals));
    TRY(dg_copy_to_device(g->e, g->d_vid, val_id, n_vals * 8));
    TRY(dg_copy_to_device(g->e, g->d_vh, val_hash, n_vals * 8));
    g->th_vals = n_vals;
  }
  g->th_stale = 0;
  g->th.node_hash = g->d_nh;
  g->th.n_nodes = g->th_nodes;
  g->th.val_id = g->d_vid;
  g->th.val_hash = g->d_vh;
  g->th.n_vals = g->th_vals;
  return DG_OK;
}

int dgr_remap(dgr_engine* g, const uint64_t* old_ids, const uint64_t* new_ids, uint64_t n) {
  if (!g || (n && (!old_ids || !new_ids))) return DG_E_INVAL;
  g->th_stale = 1; /* the value table's ids moved: re-upload before the next tree call */
  if (!n) return DG_OK;
  TRY(ri_grow_msg(g, 2 * n));
  memcpy(g->h_msg, old_ids, n * 8);
  memcpy(g->h_msg + n, new_ids, n * 8);
  TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, 2 * n * 8));
  for (dgr_state* s = g->live; s; s = s->next)
    TRY(dg_remap_values(g->e, &s->rows, g->d_msg, g->d_msg + n, n));
  return DG_OK;
}

int dgr_sweep(dgr_engine* g, int column, const uint64_t* ids, uint64_t n_ids, const uint8_t** used,
              uint64_t* n_used, uint64_t* n_unknown) {
  if (!g || !used || !n_used || (n_ids && !ids)) return DG_E_INVAL;
  *used = NULL;
  *n_used = 0;
  if (g->n_live > g->sw_cap) {
    const uint64_t want = umax(g->n_live, 2 * g->sw_cap) + 4;
    dg_store* q = (dg_store*)realloc(g->sw_stores, want * sizeof *q);
    if (!q) return DG_E_NOMEM;
    g->sw_stores = q;
    g->sw_cap = want;
  }
  uint64_t k = 0;
  for (dgr_state* s = g->live; s; s = s->next) g->sw_stores[k++] = s->rows;
  /* the table goes down in the message buffer; the flags come home at the head of the return
   * block (page-locked: the kernel writes them there, no copy and no second wait) */
  TRY(ri_grow_msg(g, n_ids + 1));
  TRY(ri_grow_back(g, rp_back_s_for_bytes(n_ids), 0));
  if (n_ids) {
    memcpy(g->h_msg, ids, n_ids * 8);
    TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, n_ids * 8));
  }
  TRY(dg_mark_ids(g->e, g->sw_stores, k, column, g->d_msg, n_ids, (uint8_t*)g->h_back, n_used, n_unknown));
  /* the caller drops table entries by these flags: the device copies of the value table are
   * re-uploaded before the next tree call (the key table has no device copy) */
  if (column == DG_COL_VAL) g->th_stale = 1;
  *used = (const uint8_t*)g->h_back;
  return DG_OK;
}

/* ------------------------------------------------------------ states */
static void link_state(dgr_engine* g, dgr_state* s) {
  s->next = g->live;
  if (g->live) g->live->prev = s;
  g->live = s;
  g->n_live++;
}

void ri_free_tree(dgr_state* s) {
  dg_engine* e = s->g->e;
  if (s->has_tree || s->tree.nodes) {
    dg_buffer_free(e, s->tree.nodes);
    dg_buffer_free(e, s->tree.counts);
    dg_buffer_free(e, s->tree.starts);
  }
  memset(&s->tree, 0, sizeof s->tree);
  s->has_tree = 0;
}

int dgr_state_free(dgr_state* s) {
  if (!s) return DG_OK;
  dgr_engine* g = s->g;
  if (s->prev) s->prev->next = s->next; else g->live = s->next;
  if (s->next) s->next->prev = s->prev;
  g->n_live--;
  dg_store_free(g->e, &s->rows);
  dg_store_free(g->e, &s->spare);
  dg_context_free(g->e, &s->ctx);
  ri_free_tree(s);
  free(s);
  return DG_OK;
}

int dgr_state_load(dgr_engine* g, const dg_store* rows, const dg_context* ctx, dgr_state** out) {
  if (!g || !rows || !ctx || !out) return DG_E_INVAL;
  *out = NULL;
  dgr_state* s = (dgr_state*)calloc(1, sizeof *s);
  if (!s) return DG_E_NOMEM;
  s->g = g;
  link_state(g, s);
  int rc = dg_store_alloc(g->e, umax(rows->n, 1), &s->rows);
  if (!rc) rc = dg_context_alloc(g->e, umax(2 * ctx->n, 16), &s->ctx);
  if (!rc) rc = ri_grow_msg(g, rows_words(rows->n) + ctx_words(ctx->n));
  dg_store rv;
  dg_context cv;
  if (!rc) {
    const uint64_t o = rp_pack_rows(g->h_msg, g->d_msg, 0, rows, &rv);
    const uint64_t w = rp_pack_ctx(g->h_msg, g->d_msg, o, ctx, &cv);
    rc = dg_copy_async(g->e, g->d_msg, g->h_msg, w * 8);
  }
  /* the map walk's order -> the store's (the radix sort also drops exact duplicates) */
  if (!rc && rows->n) rc = dg_sort_store(g->e, &rv, &s->rows);
  if (!rc && ctx->n) rc = dg_sort_context(g->e, &cv, &s->ctx);
  s->ctx.kind = ctx->kind;
  if (!rc && !ctx->n) s->ctx.n = 0;
  if (rc) {
    dgr_state_free(s);
    return rc;
  }
  s->version = 1;
  *out = s;
  return DG_OK;
}

uint64_t dgr_state_version(const dgr_state* s) { return s ? s->version : 0; }
uint64_t dgr_state_rows(const dgr_state* s) { return s ? s->rows.n : 0; }
int dgr_state_has_tree(const dgr_state* s) { return s ? s->has_tree : 0; }
