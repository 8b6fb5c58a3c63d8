/*
 * replica_pack.c — the replica layer's host layouts (replica_pack.h) and the public host
 * packers of replica.h.  It calls nothing in libdeltagpu and links with no library.
 */
#include "replica_pack.h"

#include <stdlib.h>
#include <string.h>

#include "replica.h"

/* ------------------------------------------------------------ views */
dg_store rp_rows(uint64_t* b, uint64_t w, uint64_t n, uint64_t cap) {
  dg_store v = {b, b + w, (int64_t*)(b + 2 * w), (uint32_t*)(b + 4 * w), b + 3 * w, n, cap};
  return v;
}

dg_context rp_ctx(uint64_t* b, uint64_t w, int32_t kind, uint64_t n, uint64_t cap) {
  dg_context v = {kind, 0, (uint32_t*)(b + w), b, n, cap};
  return v;
}

/* ------------------------------------------------------------ host packing */
static int cmp_u64(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

uint64_t rp_sort_unique(const uint64_t* keys, uint64_t n, uint64_t* dst) {
  if (n) memcpy(dst, keys, n * 8);
  qsort(dst, n, 8, cmp_u64);
  uint64_t m = 0;
  for (uint64_t i = 0; i < n; i++)
    if (!m || dst[m - 1] != dst[i]) dst[m++] = dst[i];
  return m;
}

int rp_rows_sorted(const dg_store* s) {
  for (uint64_t i = 1; i < s->n; i++) {
    const uint64_t a[5] = {s->key[i - 1], s->val[i - 1], (uint64_t)s->ts[i - 1] ^ (UINT64_C(1) << 63),
                           s->node[i - 1], s->cnt[i - 1]};
    const uint64_t b[5] = {s->key[i], s->val[i], (uint64_t)s->ts[i] ^ (UINT64_C(1) << 63), s->node[i],
                           s->cnt[i]};
    int c = 0;
    for (int f = 0; f < 5 && !c; f++) c = a[f] < b[f] ? -1 : a[f] > b[f];
    if (c >= 0) return 0;
  }
  return 1;
}

int rp_ctx_sorted(const dg_context* c) {
  for (uint64_t i = 1; i < c->n; i++) {
    if (c->node[i - 1] > c->node[i]) return 0;
    if (c->node[i - 1] == c->node[i] && (c->kind == DG_CTX_VV || c->cnt[i - 1] >= c->cnt[i])) return 0;
  }
  return 1;
}

uint64_t rp_pack_rows(uint64_t* hb, uint64_t* db, uint64_t o, const dg_store* r, dg_store* dev) {
  const uint64_t n = r->n;
  const dg_store h = rp_rows(hb + o, even(n), n, n);
  if (n) {
    memcpy(h.key, r->key, n * 8);
    memcpy(h.val, r->val, n * 8);
    memcpy(h.ts, r->ts, n * 8);
    memcpy(h.cnt, r->cnt, n * 8);
    memcpy(h.node, r->node, n * 4);
  }
  *dev = rp_rows(db + o, even(n), n, n);
  return o + rows_words(n);
}

uint64_t rp_pack_ctx(uint64_t* hb, uint64_t* db, uint64_t o, const dg_context* c, dg_context* dev) {
  const uint64_t n = c->n;
  const dg_context h = rp_ctx(hb + o, even(n), c->kind, n, n);
  if (n) {
    memcpy(h.cnt, c->cnt, n * 8);
    memcpy(h.node, c->node, n * 4);
  }
  *dev = rp_ctx(db + o, even(n), c->kind, n, n);
  return o + ctx_words(n);
}

/* The packed message of a batch of m ops (dgr_mutate_batch): key | val | ts | add_rank, m words
 * each, then the kinds, a byte each -- the ops stably sorted by key (batch order within a key),
 * an add's rank the number of adds before it in the batch, a remove's value and ts zero. */
uint64_t dgr_mutate_words(uint64_t m) { return 4 * m + (m + 7) / 8; }

typedef struct {
  uint64_t key;
  uint64_t idx;
} kidx;

static int cmp_kidx(const void* a, const void* b) { /* by key, then batch order: stable */
  const kidx *x = (const kidx*)a, *y = (const kidx*)b;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  return x->idx < y->idx ? -1 : x->idx > y->idx;
}

int dgr_mutate_pack(uint64_t* host, uint64_t m, const uint8_t* kind, const uint64_t* key, const uint64_t* val,
                    const int64_t* ts, uint64_t* n_adds) {
  kidx* ord = (kidx*)malloc((m ? m : 1) * sizeof *ord);
  uint64_t* rank = (uint64_t*)malloc((m ? m : 1) * 8);
  if (!ord || !rank) {
    free(ord);
    free(rank);
    return DG_E_NOMEM;
  }
  uint64_t adds = 0;
  for (uint64_t i = 0; i < m; i++) { /* the adds before each op, in batch order */
    ord[i].key = key[i];
    ord[i].idx = i;
    rank[i] = adds;
    adds += kind[i] != 0;
  }
  qsort(ord, m, sizeof *ord, cmp_kidx);
  uint8_t* hk = (uint8_t*)(host + 4 * m);
  for (uint64_t j = 0; j < m; j++) {
    const uint64_t i = ord[j].idx;
    host[j] = key[i];
    host[m + j] = kind[i] ? val[i] : 0;
    host[2 * m + j] = kind[i] ? (uint64_t)ts[i] : 0;
    host[3 * m + j] = rank[i];
    hk[j] = kind[i] != 0;
  }
  free(ord);
  free(rank);
  *n_adds = adds;
  return DG_OK;
}

/* The packed message of a batch of k deltas: per delta its rows | its context | its keyset
 * (sorted, unique, padded to an even number of words), every part at a 16-byte aligned
 * offset. */
uint64_t dgr_batch_words(int k, const dg_store* deltas, const dg_context* ctxs, const uint64_t* n_keys) {
  uint64_t w = 0;
  for (int i = 0; i < k; i++) w += rows_words(deltas[i].n) + ctx_words(ctxs[i].n) + even(n_keys[i]);
  return w;
}

uint64_t dgr_batch_pack(uint64_t* host, uint64_t* dev, int k, const dg_store* deltas, const dg_context* ctxs,
                        const uint64_t* const* keys, const uint64_t* n_keys, dg_store* rows_v,
                        dg_context* ctx_v, const uint64_t** keys_v, uint64_t* n_keys_v) {
  uint64_t o = 0;
  for (int i = 0; i < k; i++) {
    o = rp_pack_rows(host, dev, o, &deltas[i], &rows_v[i]);
    o = rp_pack_ctx(host, dev, o, &ctxs[i], &ctx_v[i]);
    n_keys_v[i] = rp_sort_unique(keys[i], n_keys[i], host + o);
    keys_v[i] = dev + o;
    o += even(n_keys[i]);
  }
  return o;
}

/* The packed message of k keysets (dgr_take_batch): keyset i sorted and unique at the even
 * word offset Σ_{j<i} even(n_keys[j]). */
uint64_t dgr_takes_words(int k, const uint64_t* n_keys) {
  uint64_t w = 0;
  for (int i = 0; i < k; i++) w += even(n_keys[i]);
  return w;
}

uint64_t dgr_takes_pack(uint64_t* host, uint64_t* dev, int k, const uint64_t* const* keys, const uint64_t* n_keys,
                        const uint64_t** keys_v, uint64_t* n_keys_v) {
  uint64_t o = 0;
  for (int i = 0; i < k; i++) {
    /* a Merkle conversation names its keys in ascending id order: such a keyset is copied
     * (one pass), any other sorted */
    uint64_t j = 1;
    while (j < n_keys[i] && keys[i][j - 1] < keys[i][j]) j++;
    if (j >= n_keys[i]) {
      if (n_keys[i]) memcpy(host + o, keys[i], n_keys[i] * 8);
      n_keys_v[i] = n_keys[i];
    } else {
      n_keys_v[i] = rp_sort_unique(keys[i], n_keys[i], host + o);
    }
    keys_v[i] = dev + o;
    o += even(n_keys[i]);
  }
  return o;
}

/* ------------------------------------------------------------ the continuation's frame */
uint8_t* rp_cont_write_head(uint8_t* bin, uint32_t level, uint64_t n, uint64_t n_buckets) {
  memcpy(bin, &level, 4);
  memcpy(bin + 4, &n, 8);
  memcpy(bin + 12, &n_buckets, 8);
  return bin + RP_CONT_HEAD;
}

int rp_cont_parse(const uint8_t* bin, uint64_t len, uint32_t* level, uint64_t* n, uint64_t* n_buckets) {
  if (len < RP_CONT_HEAD) return DG_E_INVAL;
  memcpy(level, bin, 4);
  memcpy(n, bin + 4, 8);
  memcpy(n_buckets, bin + 12, 8);
  if (*n > (len - RP_CONT_HEAD) / 16 || len != RP_CONT_HEAD + 16 * *n + 8 * *n_buckets) return DG_E_INVAL;
  return DG_OK;
}

dg_merkle_cont rp_cont_at(uint64_t* base, uint32_t level, uint64_t n, uint64_t n_buckets) {
  dg_merkle_cont c = {level, 0, base, base + n, n, n, base + 2 * n, n_buckets, n_buckets};
  return c;
}
