/*
 * replica_merkle.c — a state's Merkle tree and the anti-entropy conversation (replica.h):
 * dgr_merkle_build, dgr_merkle_prepare, dgr_merkle_continue (the bytes: replica_pack.h rp_cont_*).
 */
#include "replica_int.h"

/* floors of 16, no doubling; c->cap is zero unless pos and hash both stand */
static int grow_cont(dgr_engine* g, dg_merkle_cont* c, uint64_t cap, uint64_t cap_b) {
  if (!c->pos || c->cap < cap) {
    TRY(ri_renew(g, NULL, &c->hash, &c->cap, umax(cap, 16), umax(cap, 16)));
    TRY(ri_renew(g, NULL, &c->pos, &c->cap, umax(cap, 16), umax(cap, 16)));
  }
  if (!c->bucket || c->cap_buckets < cap_b)
    TRY(ri_renew(g, NULL, &c->bucket, &c->cap_buckets, umax(cap_b, 16), umax(cap_b, 16)));
  return DG_OK;
}

int dgr_merkle_build(dgr_state* s, uint64_t version, uint32_t depth) {
  if (!s || depth < 1 || depth > 28) return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  ri_free_tree(s);
  dg_merkle* t = &s->tree;
  t->depth = depth;
  t->terms = &g->th; /* rows hashed through their terms: comparable across BEAM nodes */
  int rc = dg_buffer_alloc(g->e, ((UINT64_C(2) << depth) - 1) * 8, (void**)&t->nodes);
  if (!rc) rc = dg_buffer_alloc(g->e, umax(UINT64_C(1) << depth, 16) * 2, (void**)&t->counts);
  if (!rc) rc = dg_buffer_alloc(g->e, (dg_merkle_chunks(depth) + 1) * 8, (void**)&t->starts);
  if (!rc) rc = dg_merkle_build(g->e, &s->rows, t);
  if (rc) {
    ri_free_tree(s);
    return rc;
  }
  s->has_tree = 1;
  return DG_OK;
}

#define CONT_SMALL_OUT 65536 /* entries of an outgoing continuation / keys kept in host memory */

/* a continuation in host memory (the kernel wrote it there, or it was staged there) framed as
 * the message */
static int frame_cont(dgr_engine* g, const dg_merkle_cont* co, const uint8_t** bin, uint64_t* len) {
  const uint64_t bytes = rp_cont_bytes(co->n, co->n_buckets);
  if (g->bin_cap < bytes) {
    uint8_t* p = (uint8_t*)realloc(g->h_bin, bytes);
    if (!p) return DG_E_NOMEM;
    g->h_bin = p;
    g->bin_cap = bytes;
  }
  uint8_t* data = rp_cont_write_head(g->h_bin, co->level, co->n, co->n_buckets);
  memcpy(data, co->pos, 8 * co->n);
  memcpy(data + 8 * co->n, co->hash, 8 * co->n);
  if (co->n_buckets) memcpy(data + 16 * co->n, co->bucket, 8 * co->n_buckets);
  *bin = g->h_bin;
  *len = bytes;
  return DG_OK;
}

/* a device continuation -> bytes */
static int cont_to_bytes(dgr_engine* g, const dg_merkle_cont* c, const uint8_t** bin, uint64_t* len) {
  /* staged 8-byte aligned in page-locked memory (one wait), then framed */
  TRY(ri_grow(g, &g->h_cstage, NULL, &g->h_cstage_cap, umax(2 * c->n + c->n_buckets, 1)));
  const dg_merkle_cont st = rp_cont_at(g->h_cstage, c->level, c->n, c->n_buckets);
  TRY(dg_copy_async(g->e, st.pos, c->pos, c->n * 8));
  TRY(dg_copy_async(g->e, st.hash, c->hash, c->n * 8));
  TRY(dg_copy_async(g->e, st.bucket, c->bucket, c->n_buckets * 8));
  TRY(dg_engine_sync(g->e));
  return frame_cont(g, &st, bin, len);
}

int dgr_merkle_prepare(dgr_state* s, uint64_t version, uint32_t levels, const uint8_t** bin, uint64_t* len) {
  if (!s || !bin || !len || !s->has_tree) return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  const uint32_t L = levels < s->tree.depth ? levels : s->tree.depth;
  const uint64_t n = UINT64_C(1) << L;
  if (n <= CONT_SMALL_OUT) { /* written by the kernel into page-locked memory: framed here */
    TRY(ri_grow(g, &g->h_cstage, NULL, &g->h_cstage_cap, 2 * n));
    dg_merkle_cont co;
    memset(&co, 0, sizeof co);
    co.pos = g->h_cstage;
    co.hash = g->h_cstage + n;
    co.cap = n;
    TRY(dg_merkle_prepare(g->e, &s->tree, levels, &co));
    return frame_cont(g, &co, bin, len);
  }
  TRY(grow_cont(g, &g->co, n, 1));
  g->co.n = g->co.n_buckets = 0;
  TRY(dg_merkle_prepare(g->e, &s->tree, levels, &g->co));
  return cont_to_bytes(g, &g->co, bin, len);
}

/* One hop through dg_merkle_continue_home: the incoming continuation read where it was
 * unpacked (mapped memory), the next one (truncated to max_sync) or the keys written by
 * the kernel into page-locked memory, one launch and one wait.  *done = 0: over its
 * limits (nothing happened; the general path runs). */
static int continue_small(dgr_state* s, uint32_t level, uint64_t n, uint64_t nb, uint32_t levels,
                          uint64_t max_sync, int* status, const uint8_t** out_bin, uint64_t* out_len,
                          const uint64_t** keys, uint64_t* n_keys, int* done) {
  dgr_engine* g = s->g;
  *done = 0;
  static int general = -1; /* DGR_CONT_GENERAL=1: always the general calls (A/B) */
  if (general < 0) general = getenv("DGR_CONT_GENERAL") != NULL;
  const uint32_t depth = s->tree.depth;
  if (general || n > DG_CONT_HOME_ENTRIES || nb > DG_CONT_HOME_BUCKETS || level > depth + 1) return DG_OK;
  const dg_merkle_cont ci = rp_cont_at(g->h_msg, level, n, nb);
  uint64_t C, CB = umax(umin(n, max_sync), 1);
  if (level < depth) {
    const uint32_t k = levels < depth - level ? levels : depth - level;
    C = umin(n << k, max_sync);
  } else {
    C = umax(4 * umin(n, max_sync), 64);
  }
  C = umax(C, 1);
  const uint64_t kcap = umax(umin(umin(max_sync, s->rows.n + n + 1), CONT_SMALL_OUT), 1);
  TRY(ri_grow(g, &g->h_ckeys, NULL, &g->h_ckeys_cap, kcap));
  uint64_t nk = 0, ntot = 0;
  dg_merkle_cont co;
  for (int attempt = 0;; attempt++) {
    if (C > CONT_SMALL_OUT) return DG_OK;
    TRY(ri_grow(g, &g->h_cstage, NULL, &g->h_cstage_cap, 2 * C + CB));
    memset(&co, 0, sizeof co);
    co.pos = g->h_cstage;
    co.hash = g->h_cstage + C;
    co.bucket = g->h_cstage + 2 * C;
    co.cap = C;
    co.cap_buckets = CB;
    const int rc = dg_merkle_continue_home(g->e, &s->tree, &s->rows, &ci, levels, max_sync, &co, g->h_ckeys,
                                           kcap, &nk, &ntot, status);
    if (rc == DG_E_CAPACITY && attempt == 0) {
      C = umax(co.n, C);
      CB = umax(co.n_buckets, CB);
      continue;
    }
    TRY(rc);
    break;
  }
  if (*status == DG_CONT_DECLINED) return DG_OK;
  if (*status == 0) {
    if (ntot > nk && nk < max_sync) return DG_OK; /* more keys than kept here: the general path */
    *keys = g->h_ckeys;
    *n_keys = nk;
    *done = 1;
    return DG_OK;
  }
  TRY(frame_cont(g, &co, out_bin, out_len));
  *done = 1;
  return DG_OK;
}

int dgr_merkle_continue(dgr_state* s, uint64_t version, const uint8_t* bin, uint64_t len, uint32_t levels,
                        uint64_t max_sync, int* status, const uint8_t** out_bin, uint64_t* out_len,
                        const uint64_t** keys, uint64_t* n_keys) {
  if (!s || !bin || !status || !out_bin || !out_len || !keys || !n_keys || !s->has_tree || len < RP_CONT_HEAD)
    return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  uint32_t level;
  uint64_t n, nb;
  TRY(rp_cont_parse(bin, len, &level, &n, &nb));
  *status = 0;
  *n_keys = 0;
  *out_bin = NULL;
  *out_len = 0;
  /* the incoming continuation as ONE copy: pos | hash | bucket in the message buffer */
  TRY(ri_grow_msg(g, 2 * n + nb + 1));
  if (2 * n + nb) memcpy(g->h_msg, bin + RP_CONT_HEAD, (2 * n + nb) * 8);
  int done = 0;
  TRY(continue_small(s, level, n, nb, levels, max_sync, status, out_bin, out_len, keys, n_keys, &done));
  if (done) return DG_OK;
  *status = 0;
  TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, (2 * n + nb) * 8));
  const dg_merkle_cont ci = rp_cont_at(g->d_msg, level, n, nb);
  /* keys: max_sync of them (UINT64_MAX, :infinite -- at most every key of both sides) */
  const uint64_t cap_keys = umax(umin(max_sync, s->rows.n + n + 1), 1);
  TRY(ri_grow(g, NULL, &g->d_ckeys, &g->ckeys_cap, cap_keys));
  uint64_t cap = 4 * umax(n, 1), cap_b = umax(n, 1), nk = 0, ntot = 0;
  int rc = DG_OK;
  for (int attempt = 0; attempt < 3; attempt++) {
    TRY(grow_cont(g, &g->co, cap, cap_b));
    g->co.n = g->co.n_buckets = 0;
    rc = dg_merkle_continue(g->e, &s->tree, &s->rows, &ci, levels, &g->co, g->d_ckeys, cap_keys, &nk, &ntot,
                            status);
    if (rc != DG_E_CAPACITY) break;
    cap = umax(g->co.n, cap);
    cap_b = umax(g->co.n_buckets, cap_b);
  }
  TRY(rc);
  if (*status == 1) {
    if (max_sync != UINT64_MAX) TRY(dg_merkle_truncate(g->e, &s->tree, &g->co, max_sync)); /* :98 */
    return cont_to_bytes(g, &g->co, out_bin, out_len);
  }
  /* {:ok, keys}: the first max_sync_size differing keys (Enum.take, :105) */
  TRY(ri_grow(g, &g->h_ckeys, NULL, &g->h_ckeys_cap, umax(nk, 1)));
  TRY(dg_copy_async(g->e, g->h_ckeys, g->d_ckeys, nk * 8));
  TRY(dg_engine_sync(g->e));
  *keys = g->h_ckeys;
  *n_keys = nk;
  return DG_OK;
}
