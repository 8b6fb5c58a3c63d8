/*
 * replica_take.c — the calls that read a state (replica.h): dgr_read, dgr_take and
 * dgr_take_batch.  Versions do not move.
 */
#include "replica_int.h"

int dgr_read(dgr_state* s, uint64_t version, int all, const uint64_t* keys, uint64_t n_keys,
             const uint64_t** out_key, const uint64_t** out_val, uint64_t* n_out) {
  if (!s || !out_key || !out_val || !n_out || (!all && n_keys && !keys)) return DG_E_INVAL;
  TRY(check_version(s, version));
  dgr_engine* g = s->g;
  *n_out = 0;
  uint64_t nk = 0;
  if (!all) {
    TRY(ri_grow_msg(g, n_keys + 1));
    nk = rp_sort_unique(keys, n_keys, g->h_msg);
    TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, nk * 8));
  }
  const uint64_t cap = umax(all ? s->rows.n : umin(nk, s->rows.n), 1);
  TRY(ri_grow(g, NULL, &g->d_rd, &g->rd_cap, 2 * cap));
  TRY(ri_grow(g, &g->h_rd, NULL, &g->h_rd_cap, g->rd_cap));
  const uint64_t half = g->rd_cap / 2;
  *out_key = g->h_rd;
  *out_val = g->h_rd + half;
  if (s->rows.n == 0 || (!all && nk == 0)) return DG_OK;
  uint64_t n = 0;
  if (half <= 65536) {
    /* a small read: the kernels write the page-locked output directly (it is mapped into
     * the device's address space), so the read's own wait is the only one */
    TRY(dg_read_lww(g->e, &s->rows, all ? NULL : g->d_msg, nk, g->h_rd, g->h_rd + half, half, &n));
  } else {
    TRY(dg_read_lww(g->e, &s->rows, all ? NULL : g->d_msg, nk, g->d_rd, g->d_rd + half, half, &n));
    TRY(dg_copy_async(g->e, g->h_rd, g->d_rd, n * 8));
    TRY(dg_copy_async(g->e, g->h_rd + half, g->d_rd + half, n * 8));
    TRY(dg_engine_sync(g->e));
  }
  *n_out = n;
  return DG_OK;
}

/* The rows of the m sorted, unique keys in the message taken into g->tk -- k < 0: of the ONE
 * keyset at its head (dg_take_keys); else of the batch's k keysets (dg_take_keysets), whose
 * *nu union keys, masks and offsets are copied home on the way (no wait) -- with one retry
 * at the row count the take then reports, and downloaded into h_tk as *out. */
static int take_home(dgr_state* s, int k, uint64_t m, uint64_t* nu, dg_store* out) {
  dgr_engine* g = s->g;
  const uint64_t K = g->tb_cap;
  uint64_t cap = umin(s->rows.n, 4 * m + 64);
  for (int attempt = 0;; attempt++) {
    TRY(ri_grow_store(g, &g->tk, umax(cap, 1)));
    g->tk.n = 0;
    const int rc = k < 0 ? dg_take_keys(g->e, &s->rows, g->d_msg, m, &g->tk)
                         : dg_take_keysets(g->e, &s->rows, k, g->b_keys, g->b_nk, g->d_tb, g->d_tb + K,
                                           g->d_tb + 2 * K, K, nu, &g->tk);
    if (rc == DG_E_CAPACITY && attempt == 0 && *nu <= K) { /* (one keyset: *nu stays 0) */
      cap = g->tk.n;
      continue;
    }
    TRY(rc);
    break;
  }
  if (k >= 0) { /* home: the union keys, their masks and offsets, then the rows -- each once */
    if (*nu) {
      TRY(dg_copy_async(g->e, g->h_tb, g->d_tb, *nu * 8));
      TRY(dg_copy_async(g->e, g->h_tb + K, g->d_tb + K, *nu * 8));
    }
    TRY(dg_copy_async(g->e, g->h_tb + 2 * K, g->d_tb + 2 * K, (*nu + 1) * 8));
  }
  const uint64_t n = g->tk.n;
  TRY(ri_grow(g, &g->h_tk, NULL, &g->h_tk_cap, rows_words(n) + 2));
  dg_store hv = rp_rows(g->h_tk, even(n), 0, umax(n, 1));
  TRY(dg_store_download(g->e, &g->tk, &hv));
  *out = hv;
  return DG_OK;
}

int dgr_take(dgr_state* s, uint64_t version, const uint64_t* keys, uint64_t n_keys, dg_store* out) {
  if (!s || !out || (n_keys && !keys)) return DG_E_INVAL;
  TRY(check_version(s, version));
  return ri_take(s, keys, n_keys, out);
}

int ri_take(dgr_state* s, const uint64_t* keys, uint64_t n_keys, dg_store* out) {
  dgr_engine* g = s->g;
  TRY(ri_grow_msg(g, n_keys + 1));
  const uint64_t nk = rp_sort_unique(keys, n_keys, g->h_msg);
  TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, nk * 8));
  uint64_t nu = 0;
  return take_home(s, -1, nk, &nu, out);
}

/* dgr_take_batch's key arrays for K union keys (contents not kept) */
static int grow_taken(dgr_engine* g, uint64_t K) {
  if (g->d_tb && g->tb_cap >= K) return DG_OK;
  K = umax(K, 2 * g->tb_cap) + 64;
  return ri_renew(g, &g->h_tb, &g->d_tb, &g->tb_cap, K, 3 * K + 1);
}

int dgr_take_batch(dgr_state* s, uint64_t version, int k, const uint64_t* const* keys, const uint64_t* n_keys,
                   dgr_taken* out) {
  if (!s || !out || k < 0 || k > 64 || (k && (!keys || !n_keys))) return DG_E_INVAL;
  for (int i = 0; i < k; i++)
    if (n_keys[i] && !keys[i]) return DG_E_INVAL;
  TRY(check_version(s, version));
  return ri_take_batch(s, k, keys, n_keys, out);
}

int ri_take_batch(dgr_state* s, int k, const uint64_t* const* keys, const uint64_t* n_keys, dgr_taken* out) {
  dgr_engine* g = s->g;
  /* ONE message and one copy: the k keysets, each sorted and unique */
  TRY(ri_grow_batch(g, (uint64_t)k));
  const uint64_t words = dgr_takes_words(k, n_keys);
  TRY(ri_grow_msg(g, words + 2));
  dgr_takes_pack(g->h_msg, g->d_msg, k, keys, n_keys, g->b_keys, g->b_nk);
  if (words) TRY(dg_copy_async(g->e, g->d_msg, g->h_msg, words * 8));
  uint64_t m = 0;
  for (int i = 0; i < k; i++) m += g->b_nk[i];
  TRY(grow_taken(g, m));
  uint64_t nu = 0;
  TRY(take_home(s, k, m, &nu, &out->rows));
  TRY(dg_engine_sync(g->e));
  out->n_keys = nu;
  out->keys = g->h_tb;
  out->masks = g->h_tb + g->tb_cap;
  out->offs = g->h_tb + 2 * g->tb_cap;
  return DG_OK;
}
