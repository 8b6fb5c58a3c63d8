/*
 * replica_join.c — the calls that change a state (replica.h): dgr_join_delta, dgr_join_deltas,
 * dgr_mutate_batch and their *_diffs forms, with the small path and the return block.
 */
#include "replica_int.h"

/* the spare buffer and the context's room for a union with `dn` more entries, grown */
static int room_for(dgr_state* s, uint64_t rows, uint64_t dn) {
  dgr_engine* g = s->g;
  if (s->spare.cap < s->rows.n + rows) {
    TRY(dg_store_free(g->e, &s->spare));
    TRY(dg_store_alloc(g->e, 2 * (s->rows.n + rows) + 16, &s->spare));
  }
  if (s->ctx.cap < s->ctx.n + dn) {
    dg_context nctx;
    memset(&nctx, 0, sizeof nctx);
    TRY(dg_context_alloc(g->e, 2 * (s->ctx.n + dn) + 16, &nctx));
    int rc = dg_copy_async(g->e, nctx.node, s->ctx.node, s->ctx.n * 4);
    if (!rc) rc = dg_copy_async(g->e, nctx.cnt, s->ctx.cnt, s->ctx.n * 8);
    if (rc) {
      dg_context_free(g->e, &nctx);
      return rc;
    }
    nctx.n = s->ctx.n;
    nctx.kind = s->ctx.kind;
    TRY(dg_context_free(g->e, &s->ctx)); /* (waits for the copies) */
    s->ctx = nctx;
  }
  return DG_OK;
}

/* A small delta (a local mutation, a small sync delta): dg_join_delta_home does the whole
 * update_state_with_delta in one launch chain and writes the result into page-locked
 * memory with ONE wait.  *done = 0: not small after all (nothing happened). */
static int small_fits(const dgr_state* s, const dg_store* drows, const dg_context* dctx, uint64_t n_keys) {
  return n_keys <= 512 && drows->n <= 512 && dctx->n <= 1024 && s->ctx.kind == DG_CTX_VV;
}

static void home_views(dgr_state* s, dgr_changed* out, dgr_diffs* diffs);

static int apply_small(dgr_state* s, const dg_store* drows, const dg_context* dctx, const uint64_t* dkeys,
                       uint64_t n_keys, dgr_changed* out, dgr_diffs* diffs, int* done) {
  dgr_engine* g = s->g;
  *done = 0;
  if (!small_fits(s, drows, dctx, n_keys)) return DG_OK;
  if (!g->h_home) TRY(dg_host_alloc(g->e, DG_HOME_DIFFS_WORDS * 8, (void**)&g->h_home));
  int swapped = 0;
  /* (diffs: the LWW reads before and after come out of the same kernel, the same wait) */
  const int rc = (diffs ? dg_join_delta_home_diffs : dg_join_delta_home)(
      g->e, &s->rows, &s->ctx, drows, dctx, dkeys, n_keys, &s->spare, s->has_tree ? &s->tree : NULL, g->h_home,
      &swapped);
  if (rc) {
    s->version++;
    return rc;
  }
  uint64_t* h = g->h_home;
  if (h[0] & DG_HOME_FALLBACK) return DG_OK;
  s->version++;
  *done = 1;
  home_views(s, out, diffs);
  return DG_OK;
}

/* the result block of a served home call (the join's or the mutation's) as the caller's views */
static void home_views(dgr_state* s, dgr_changed* out, dgr_diffs* diffs) {
  uint64_t* h = s->g->h_home;
  out->version = s->version;
  out->n_changed = h[1];
  out->keys = h + DG_HOME_KEYS;
  out->rows = rp_rows(h + DG_HOME_ROWS, DG_HOME_STRIDE, h[2], DG_HOME_STRIDE);
  out->ctx = rp_ctx(h + DG_HOME_CTX, DG_HOME_NODES, DG_CTX_VV, h[3], DG_HOME_NODES);
  if (diffs)
    *diffs = (dgr_diffs){h[1], h + DG_HOME_DIFF_OLD, h + DG_HOME_DIFF_NEW, (const uint8_t*)(h + DG_HOME_DIFF_FLAGS)};
}

/* The return block's views a join writes through: the changed keys' rows, the joined
 * context, the diff arrays (the changed keys themselves stand at the block's head). */
typedef struct {
  dg_store tk;
  dg_context co;
  dg_lww_diffs dd;
} back_views;

/* the return block grown for S keys / rows and a context of C entries (g->back_s and
 * g->back_c may be larger), and its views */
static int open_back(dgr_engine* g, uint64_t S, uint64_t C, back_views* v) {
  TRY(ri_grow_back(g, S, C));
  v->tk = rp_back_rows(g->h_back, g->back_s);
  v->co = rp_back_ctx(g->h_back, g->back_s, g->back_c);
  v->dd = rp_back_diffs(g->h_back, g->back_s, g->back_c);
  return DG_OK;
}

/* the state's context copied home into the return block's (one wait) */
static int ctx_home(dgr_state* s, dg_context* co) {
  dgr_engine* g = s->g;
  TRY(dg_copy_async(g->e, co->cnt, s->ctx.cnt, s->ctx.n * 8));
  TRY(dg_copy_async(g->e, co->node, s->ctx.node, s->ctx.n * 4));
  TRY(dg_engine_sync(g->e));
  co->n = s->ctx.n;
  co->kind = s->ctx.kind;
  return DG_OK;
}

/* What a join wrote into the return block (n_changed keys at its head, v as the call left
 * it) as the caller's views.  Rows or a context past the block: the changed keys (and their
 * diffs) are parked, the block grown, the rows taken from the joined state and the context
 * copied (the kernels write the page-locked block directly). */
static int bring_home(dgr_state* s, uint64_t n_changed, back_views* v, dgr_changed* out, dgr_diffs* diffs) {
  dgr_engine* g = s->g;
  if (v->tk.n > v->tk.cap || v->co.n > v->co.cap) {
    TRY(ri_grow_msg(g, diffs ? 3 * n_changed + (n_changed + 7) / 8 + 1 : n_changed + 1)); /* (+ the flags' words) */
    memcpy(g->h_msg, rp_back_keys(g->h_back), n_changed * 8);
    if (diffs) {
      memcpy(g->h_msg + n_changed, v->dd.old_val, n_changed * 8);
      memcpy(g->h_msg + 2 * n_changed, v->dd.new_val, n_changed * 8);
      memcpy(g->h_msg + 3 * n_changed, v->dd.flags, n_changed);
    }
    TRY(open_back(g, umax(v->tk.n, n_changed), s->ctx.n, v));
    memcpy(rp_back_keys(g->h_back), g->h_msg, n_changed * 8);
    if (diffs) {
      memcpy(v->dd.old_val, g->h_msg + n_changed, n_changed * 8);
      memcpy(v->dd.new_val, g->h_msg + 2 * n_changed, n_changed * 8);
      memcpy(v->dd.flags, g->h_msg + 3 * n_changed, n_changed);
    }
    TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, n_changed * 8));
    TRY(dg_take_keys(g->e, &s->rows, g->d_msg, n_changed, &v->tk));
    TRY(ctx_home(s, &v->co));
  }
  out->version = s->version;
  out->n_changed = n_changed;
  out->keys = rp_back_keys(g->h_back);
  out->rows = v->tk; /* (the calls set n, and the context's kind, in the block's views) */
  out->ctx = v->co;
  if (diffs) *diffs = (dgr_diffs){n_changed, v->dd.old_val, v->dd.new_val, v->dd.flags};
  return DG_OK;
}

/* The join of a delta on the device (rows and context sorted, keys ascending unique) into
 * the state, and the result brought home with one wait.  try_small: the small join first. */
static int apply_delta(dgr_state* s, const dg_store* drows, const dg_context* dctx, const uint64_t* dkeys,
                       uint64_t n_keys, dgr_changed* out, dgr_diffs* diffs, int try_small) {
  dgr_engine* g = s->g;
  TRY(room_for(s, drows->n, dctx->n));
  if (try_small) {
    int done = 0;
    TRY(apply_small(s, drows, dctx, dkeys, n_keys, out, diffs, &done));
    if (done) return DG_OK;
  }
  /* the changed keys, their rows and the joined context straight into the page-locked
   * block (dg_join_delta_out: the kernels write it, one wait); rows of the changed keys
   * past the block (a key with several entries) are taken afterwards */
  back_views v;
  TRY(open_back(g, 2 * n_keys + 64, s->ctx.n + dctx->n, &v));
  uint64_t* hb = rp_back_keys(g->h_back);
  uint64_t n_changed = 0;
  int swapped = 0;
  const int rc = diffs ? dg_join_delta_diffs(g->e, &s->rows, &s->ctx, drows, dctx, dkeys, n_keys, &s->spare,
                                             s->has_tree ? &s->tree : NULL, hb, g->back_s, &n_changed, &swapped,
                                             &v.tk, &v.co, &v.dd)
                       : dg_join_delta_out(g->e, &s->rows, &s->ctx, drows, dctx, dkeys, n_keys, &s->spare,
                                           s->has_tree ? &s->tree : NULL, hb, g->back_s, &n_changed, &swapped,
                                           &v.tk, &v.co);
  s->version++; /* applied, or failed: either way no older struct reads the device again */
  TRY(rc);
  if (diffs && v.dd.cap == 0 && n_changed) {
    /* the gather behind the committed join failed (deltagpu.h): the old rows survive only
     * where the join went through the spare store, which still describes them */
    if (!swapped) return DG_E_DEVICE;
    v.dd = rp_back_diffs(g->h_back, g->back_s, g->back_c);
    TRY(dg_read_diff(g->e, &s->spare, &s->rows, hb, n_changed, &v.dd));
  }
  return bring_home(s, n_changed, &v, out, diffs);
}

/* dgr_join_delta (diffs NULL) and dgr_join_delta_diffs */
static int join_delta(dgr_state* s, uint64_t version, const dg_store* delta, const dg_context* delta_ctx,
                      const uint64_t* keys, uint64_t n_keys, dgr_changed* out, dgr_diffs* diffs) {
  if (!s || !delta || !delta_ctx || !out || (n_keys && !keys)) return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  /* ONE message: rows | context | keyset (sorted, unique) */
  TRY(ri_grow_msg(g, rows_words(delta->n) + ctx_words(delta_ctx->n) + n_keys + 2));
  dg_store rv;
  dg_context cv;
  const uint64_t oc = rp_pack_rows(g->h_msg, g->d_msg, 0, delta, &rv);
  const uint64_t o = rp_pack_ctx(g->h_msg, g->d_msg, oc, delta_ctx, &cv);
  const uint64_t nk = rp_sort_unique(keys, n_keys, g->h_msg + o);
  const int rows_ok = rp_rows_sorted(delta), ctx_ok = rp_ctx_sorted(delta_ctx);
  int try_small = 1;
  if (rows_ok && ctx_ok && small_fits(s, delta, delta_ctx, nk)) {
    /* a mutation or a small sync delta: the small join reads the message where the host
     * packed it (page-locked, mapped memory: the host twins of rv, at word 0, and cv, at oc)
     * -- no copy launch; declined, the general path copies it */
    const dg_store hr = rp_rows(g->h_msg, even(rv.n), rv.n, rv.cap);
    const dg_context hc = rp_ctx(g->h_msg + oc, even(cv.n), cv.kind, cv.n, cv.cap);
    TRY(room_for(s, delta->n, delta_ctx->n));
    int done = 0;
    TRY(apply_small(s, &hr, &hc, g->h_msg + o, nk, out, diffs, &done));
    if (done) return DG_OK;
    try_small = 0;
  }
  TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, (o + nk) * 8));
  const dg_store* dr = &rv;
  const dg_context* dc = &cv;
  if (!rows_ok) { /* a map walk of more than 32 keys: HAMT order */
    TRY(ri_grow_store(g, &g->drows, delta->n));
    TRY(dg_sort_store(g->e, &rv, &g->drows));
    dr = &g->drows;
  }
  if (!ctx_ok) {
    TRY(ri_grow_ctx(g, &g->dctx, delta_ctx->n));
    TRY(dg_sort_context(g->e, &cv, &g->dctx));
    dc = &g->dctx;
  }
  return apply_delta(s, dr, dc, g->d_msg + o, nk, out, diffs, try_small);
}

int dgr_join_delta(dgr_state* s, uint64_t version, const dg_store* delta, const dg_context* delta_ctx,
                   const uint64_t* keys, uint64_t n_keys, dgr_changed* out) {
  return join_delta(s, version, delta, delta_ctx, keys, n_keys, out, NULL);
}

int dgr_join_delta_diffs(dgr_state* s, uint64_t version, const dg_store* delta, const dg_context* delta_ctx,
                         const uint64_t* keys, uint64_t n_keys, dgr_changed* out, dgr_diffs* diffs) {
  return diffs ? join_delta(s, version, delta, delta_ctx, keys, n_keys, out, diffs) : DG_E_INVAL;
}

/* dgr_sync_from (diffs NULL) and dgr_sync_from_diffs: the diff of the two trees answered with
 * src's rows of the kept keys (dg_merkle_diff_take, side 1: one launch chain, one wait) into
 * engine-owned device buffers, then apply_delta with those rows where they stand, src's context
 * as the delta's and the kept keys as the keyset.  Nothing goes through the host but counts. */
static int sync_from(dgr_state* dst, uint64_t dst_version, dgr_state* src, uint64_t src_version, uint64_t max_sync,
                     dgr_changed* out, dgr_diffs* diffs, uint64_t* n_total) {
  if (!dst || !src || !out || !n_total || dst == src || dst->g != src->g) return DG_E_INVAL;
  if (!dst->has_tree || !src->has_tree) return DG_E_INVAL;
  if (dst->tree.depth != src->tree.depth || dst->tree.shard_bits != src->tree.shard_bits ||
      dst->tree.shard != src->tree.shard)
    return DG_E_INVAL;
  TRY(check_version(dst, dst_version));
  TRY(check_version(src, src_version));
  dgr_engine* g = dst->g;
  /* at most one differing key per distinct key of either state */
  const uint64_t most = dst->tree.n_keys + src->tree.n_keys;
  const uint64_t cap = umax(max_sync ? umin(max_sync, most) : most, 1);
  TRY(ri_grow(g, NULL, &g->d_sy, &g->sy_cap, 2 * cap + 1)); /* keys [0, cap) | offs [cap, 2 cap + 1) */
  TRY(ri_grow_store(g, &g->sy_rows, umax(umin(src->rows.n, 4 * cap + 64), 1)));
  uint64_t n = 0;
  int rc = dg_merkle_diff_take(g->e, &dst->tree, &dst->rows, &src->tree, &src->rows, 1, g->d_sy, cap, g->d_sy + cap,
                               &g->sy_rows, &n, n_total);
  if (rc == DG_E_CAPACITY) { /* a key with many entries: once more with the room the call asked for */
    TRY(ri_grow_store(g, &g->sy_rows, g->sy_rows.n));
    rc = dg_merkle_diff_take(g->e, &dst->tree, &dst->rows, &src->tree, &src->rows, 1, g->d_sy, cap, g->d_sy + cap,
                             &g->sy_rows, &n, n_total);
  }
  TRY(rc);
  if (n == 0) { /* nothing differs: the context comes home, the version stays, no join */
    back_views v;
    TRY(open_back(g, 64, dst->ctx.n, &v));
    TRY(ctx_home(dst, &v.co));
    return bring_home(dst, 0, &v, out, diffs);
  }
  return apply_delta(dst, &g->sy_rows, &src->ctx, g->d_sy, n, out, diffs, 1);
}

int dgr_sync_from(dgr_state* dst, uint64_t dst_version, dgr_state* src, uint64_t src_version, uint64_t max_sync,
                  dgr_changed* out, uint64_t* n_total) {
  return sync_from(dst, dst_version, src, src_version, max_sync, out, NULL, n_total);
}

int dgr_sync_from_diffs(dgr_state* dst, uint64_t dst_version, dgr_state* src, uint64_t src_version, uint64_t max_sync,
                        dgr_changed* out, dgr_diffs* diffs, uint64_t* n_total) {
  return diffs ? sync_from(dst, dst_version, src, src_version, max_sync, out, diffs, n_total) : DG_E_INVAL;
}

/* Which batches try dg_join_deltas_keyed first (g->deltas_route, DGR_DELTAS_ROUTE at engine
 * open): `keyed` every batch, `stream` none.  `auto` is to be the region where the keyed call
 * measures faster than both the streaming call and k single joins THROUGH THIS LAYER; that
 * table does not exist yet (DESIGN 4.17 has figures of the library calls only), so auto is
 * stream. */
static int keyed_wanted(const dgr_engine* g) { return g->deltas_route == DGR_ROUTE_KEYED; }

/* dgr_join_deltas (diffs NULL) and dgr_join_deltas_diffs */
static int join_deltas(dgr_state* s, uint64_t version, int k, const dg_store* deltas, const dg_context* ctxs,
                       const uint64_t* const* keys, const uint64_t* n_keys, dgr_changed* out, dgr_diffs* diffs) {
  if (!s || !out || k < 0 || (k && (!deltas || !ctxs || !keys || !n_keys))) return DG_E_INVAL;
  for (int i = 0; i < k; i++)
    if (n_keys[i] && !keys[i]) return DG_E_INVAL;
  if (k == 1) return join_delta(s, version, &deltas[0], &ctxs[0], keys[0], n_keys[0], out, diffs);
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  /* ONE message and one copy: per delta its rows | context | keyset (sorted, unique) */
  TRY(ri_grow_batch(g, (uint64_t)k));
  const uint64_t words = dgr_batch_words(k, deltas, ctxs, n_keys);
  TRY(ri_grow_msg(g, words + 2));
  dgr_batch_pack(g->h_msg, g->d_msg, k, deltas, ctxs, keys, n_keys, g->b_rows, g->b_ctx, g->b_keys, g->b_nk);
  if (words) TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, words * 8));
  /* deltas the map walk did not give in order are sorted on the device, into one buffer
   * for all of them (each at an even row offset) */
  uint64_t n_rows = 0, n_ctx = 0, n_k = 0, un_rows = 0, un_ctx = 0;
  for (int i = 0; i < k; i++) {
    n_rows += deltas[i].n;
    n_ctx += ctxs[i].n;
    n_k += g->b_nk[i];
    g->b_unsorted[i] = (uint8_t)((rp_rows_sorted(&deltas[i]) ? 0 : 1) + (rp_ctx_sorted(&ctxs[i]) ? 0 : 2));
    if (g->b_unsorted[i] & 1) un_rows += even(deltas[i].n);
    if (g->b_unsorted[i] & 2) un_ctx += even(ctxs[i].n);
  }
  if (un_rows) TRY(ri_grow_store(g, &g->drows, un_rows));
  if (un_ctx) TRY(ri_grow_ctx(g, &g->dctx, un_ctx));
  uint64_t ro = 0, co_ = 0;
  for (int i = 0; i < k; i++) {
    if (g->b_unsorted[i] & 1) {
      const dg_store* b = &g->drows;
      dg_store v = {b->key + ro, b->val + ro, b->ts + ro, b->node + ro, b->cnt + ro, 0, deltas[i].n};
      TRY(dg_sort_store(g->e, &g->b_rows[i], &v));
      g->b_rows[i] = v;
      ro += even(deltas[i].n);
    }
    if (g->b_unsorted[i] & 2) {
      const dg_context* b = &g->dctx;
      dg_context v = {ctxs[i].kind, 0, b->node + co_, b->cnt + co_, 0, ctxs[i].n};
      TRY(dg_sort_context(g->e, &g->b_ctx[i], &v));
      v.kind = ctxs[i].kind;
      g->b_ctx[i] = v;
      co_ += even(ctxs[i].n);
    }
  }
  TRY(room_for(s, n_rows, n_ctx));
  /* a changed key is a key of a keyset or of a delta row (one carried over from outside
   * its keyset) */
  back_views v;
  TRY(open_back(g, n_k + n_rows + 64, s->ctx.n + n_ctx, &v));
  uint64_t n_changed = 0;
  if (k == 0) { /* nothing changes: the context comes home, the version stays */
    TRY(ctx_home(s, &v.co));
    return bring_home(s, 0, &v, out, diffs);
  }
  /* small sync deltas: the fold at the cost of the keys they name (dg_join_deltas_keyed); a
   * batch it declines has touched nothing and takes the streaming call */
  int rc = DG_KEYED_FALLBACK;
  if (keyed_wanted(g)) {
    int swapped = 0;
    rc = dg_join_deltas_keyed(g->e, &s->rows, &s->ctx, k, g->b_rows, g->b_ctx, g->b_keys, g->b_nk, &s->spare,
                              s->has_tree ? &s->tree : NULL, rp_back_keys(g->h_back), g->back_s, &n_changed,
                              &v.tk, &v.co, diffs ? &v.dd : NULL, &swapped);
    g->keyed_stats[DGR_KEYED_TRIED]++;
    if (rc == DG_KEYED_FALLBACK) g->keyed_stats[DGR_KEYED_DECLINED]++;
    if (rc == DG_OK) g->keyed_stats[DGR_KEYED_SERVED]++;
  }
  if (rc == DG_KEYED_FALLBACK)
    rc = dg_join_deltas(g->e, &s->rows, &s->ctx, k, g->b_rows, g->b_ctx, g->b_keys, g->b_nk, &s->spare,
                        s->has_tree ? &s->tree : NULL, rp_back_keys(g->h_back), g->back_s, &n_changed, &v.tk,
                        &v.co, diffs ? &v.dd : NULL);
  s->version++; /* applied, or failed: either way no older struct reads the device again */
  TRY(rc);
  return bring_home(s, n_changed, &v, out, diffs);
}

int dgr_join_deltas(dgr_state* s, uint64_t version, int k, const dg_store* deltas, const dg_context* ctxs,
                    const uint64_t* const* keys, const uint64_t* n_keys, dgr_changed* out) {
  return join_deltas(s, version, k, deltas, ctxs, keys, n_keys, out, NULL);
}

int dgr_join_deltas_diffs(dgr_state* s, uint64_t version, int k, const dg_store* deltas, const dg_context* ctxs,
                          const uint64_t* const* keys, const uint64_t* n_keys, dgr_changed* out,
                          dgr_diffs* diffs) {
  return diffs ? join_deltas(s, version, k, deltas, ctxs, keys, n_keys, out, diffs) : DG_E_INVAL;
}

/* Under the `home` route (g->mutate_route, DGR_MUTATE_ROUTE at engine open) a batch of at most
 * 512 ops on a VV state first tries dg_mutate_home on the message where the host packed it
 * (page-locked, mapped memory: no copy launch, no delta, one wait).  *done = 0: declined,
 * nothing happened, and the copy, dg_mutate_batch and the join run as under `batch`. */
static int mutate_home(dgr_state* s, uint32_t node, uint64_t m, uint64_t n_adds, dgr_changed* out,
                       dgr_diffs* diffs, int* done) {
  dgr_engine* g = s->g;
  *done = 0;
  if (g->mutate_route != DGR_MROUTE_HOME || m > 512 || s->ctx.kind != DG_CTX_VV) return DG_OK;
  TRY(room_for(s, m, 1));
  if (!g->h_home) TRY(dg_host_alloc(g->e, DG_HOME_DIFFS_WORDS * 8, (void**)&g->h_home));
  uint64_t* h = g->h_msg;
  int swapped = 0;
  g->mutate_stats[DGR_MUTATE_TRIED]++;
  const int rc = (diffs ? dg_mutate_home_diffs : dg_mutate_home)(
      g->e, &s->rows, &s->ctx, node, m, (const uint8_t*)(h + 4 * m), h, h + m, (const int64_t*)(h + 2 * m),
      h + 3 * m, n_adds, &s->spare, s->has_tree ? &s->tree : NULL, g->h_home, &swapped);
  if (rc) {
    s->version++;
    return rc;
  }
  if (g->h_home[0] & DG_HOME_FALLBACK) {
    g->mutate_stats[DGR_MUTATE_DECLINED]++;
    return DG_OK;
  }
  g->mutate_stats[DGR_MUTATE_SERVED]++;
  s->version++;
  *done = 1;
  home_views(s, out, diffs);
  return DG_OK;
}

/* dgr_mutate_batch (diffs NULL) and dgr_mutate_batch_diffs */
static int mutate_batch(dgr_state* s, uint64_t version, uint32_t node, uint64_t m, const uint8_t* kind,
                        const uint64_t* key, const uint64_t* val, const int64_t* ts, dgr_changed* out,
                        dgr_diffs* diffs) {
  if (!s || !out || (m && (!kind || !key || !val || !ts))) return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  /* key | val | ts | add_rank | kind, sorted by key (batch order within a key): ONE message */
  const uint64_t words = dgr_mutate_words(m);
  TRY(ri_grow_msg(g, words + 2));
  uint64_t* h = g->h_msg;
  uint64_t n_adds = 0;
  TRY(dgr_mutate_pack(h, m, kind, key, val, ts, &n_adds));
  int done = 0, rc;
  TRY(mutate_home(s, node, m, n_adds, out, diffs, &done));
  if (done) return DG_OK;
  TRY(dg_copy_async(g->e, g->d_msg, h, words * 8)); /* one copy */
  const uint64_t* d = g->d_msg;
  TRY(ri_grow_store(g, &g->mrows, umax(m, 1)));
  TRY(ri_grow(g, NULL, &g->mkeys, &g->mkeys_cap, umax(m, 1)));
  uint64_t n_keys = 0;
  for (int attempt = 0;; attempt++) {
    TRY(ri_grow_ctx(g, &g->mctx, attempt ? s->rows.n + n_adds + 1 : 8 * m + n_adds + 1));
    g->mctx.kind = DG_CTX_DOTS;
    g->mrows.n = 0;
    rc = dg_mutate_batch_async(g->e, &s->rows, &s->ctx, node, m, (const uint8_t*)(d + 4 * m), d, d + m,
                         (const int64_t*)(d + 2 * m), d + 3 * m, n_adds, &g->mrows, &g->mctx, g->mkeys,
                         g->mkeys_cap, &n_keys);
    if (rc == DG_E_CAPACITY && attempt == 0) continue;
    TRY(rc);
    break;
  }
  return apply_delta(s, &g->mrows, &g->mctx, g->mkeys, n_keys, out, diffs, 1);
}

int dgr_mutate_batch(dgr_state* s, uint64_t version, uint32_t node, uint64_t m, const uint8_t* kind,
                     const uint64_t* key, const uint64_t* val, const int64_t* ts, dgr_changed* out) {
  return mutate_batch(s, version, node, m, kind, key, val, ts, out, NULL);
}

int dgr_mutate_batch_diffs(dgr_state* s, uint64_t version, uint32_t node, uint64_t m, const uint8_t* kind,
                           const uint64_t* key, const uint64_t* val, const int64_t* ts, dgr_changed* out,
                           dgr_diffs* diffs) {
  return diffs ? mutate_batch(s, version, node, m, kind, key, val, ts, out, diffs) : DG_E_INVAL;
}
