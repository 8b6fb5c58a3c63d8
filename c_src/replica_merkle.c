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

#define CONT_SMALL_OUT RP_CONT_SMALL_OUT

/* `bytes` bytes of the engine's byte buffer from offset `at` on (what stands before is kept) */
static int bin_room(dgr_engine* g, uint64_t at, uint64_t bytes) {
  if (g->bin_cap < at + bytes) {
    const uint64_t cap = at ? umax(at + bytes, 2 * g->bin_cap) : bytes;
    uint8_t* p = (uint8_t*)realloc(g->h_bin, cap);
    if (!p) return DG_E_NOMEM;
    g->h_bin = p;
    g->bin_cap = cap;
  }
  return DG_OK;
}

/* a continuation in host memory (the kernel wrote it there, or it was staged there) framed as
 * the message, `at` bytes into the engine's byte buffer (a batch lays its frames end to end) */
static int frame_cont(dgr_engine* g, uint64_t at, const dg_merkle_cont* co, const uint8_t** bin, uint64_t* len) {
  const uint64_t bytes = rp_cont_bytes(co->n, co->n_buckets);
  TRY(bin_room(g, at, bytes));
  uint8_t* data = rp_cont_write_head(g->h_bin + at, co->level, co->n, co->n_buckets);
  memcpy(data, co->pos, 8 * co->n);
  memcpy(data + 8 * co->n, co->hash, 8 * co->n);
  if (co->n_buckets) memcpy(data + 16 * co->n, co->bucket, 8 * co->n_buckets);
  *bin = g->h_bin + at;
  *len = bytes;
  return DG_OK;
}

/* a device continuation -> bytes */
static int cont_to_bytes(dgr_engine* g, uint64_t at, const dg_merkle_cont* c, const uint8_t** bin, uint64_t* len) {
  /* staged 8-byte aligned in page-locked memory (one wait), then framed */
  TRY(ri_grow(g, &g->h_cstage, NULL, &g->h_cstage_cap, umax(2 * c->n + c->n_buckets, 1)));
  const dg_merkle_cont st = rp_cont_at(g->h_cstage, c->level, c->n, c->n_buckets);
  TRY(dg_copy_async(g->e, st.pos, c->pos, c->n * 8));
  TRY(dg_copy_async(g->e, st.hash, c->hash, c->n * 8));
  TRY(dg_copy_async(g->e, st.bucket, c->bucket, c->n_buckets * 8));
  TRY(dg_engine_sync(g->e));
  return frame_cont(g, at, &st, bin, len);
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
    return frame_cont(g, 0, &co, bin, len);
  }
  TRY(grow_cont(g, &g->co, n, 1));
  g->co.n = g->co.n_buckets = 0;
  TRY(dg_merkle_prepare(g->e, &s->tree, levels, &g->co));
  return cont_to_bytes(g, 0, &g->co, bin, len);
}

/* One hop through dg_merkle_continue_home: the incoming continuation read where it was
 * unpacked (mapped memory), the next one (truncated to max_sync) or the keys written by
 * the kernel into page-locked memory, one launch and one wait.  *done = 0: over its
 * limits (nothing happened; the general path runs). */
static int cont_general(void) { /* DGR_CONT_GENERAL=1: always the general calls (A/B) */
  static int general = -1;
  if (general < 0) general = getenv("DGR_CONT_GENERAL") != NULL;
  return general;
}

static int continue_small(dgr_state* s, uint64_t at, uint32_t level, uint64_t n, uint64_t nb, uint32_t levels,
                          uint64_t max_sync, int* status, const uint8_t** out_bin, uint64_t* out_len,
                          const uint64_t** keys, uint64_t* n_keys, int* done) {
  dgr_engine* g = s->g;
  *done = 0;
  const uint32_t depth = s->tree.depth;
  if (cont_general() || n > DG_CONT_HOME_ENTRIES || nb > DG_CONT_HOME_BUCKETS || level > depth + 1) return DG_OK;
  const dg_merkle_cont ci = rp_cont_at(g->h_msg, level, n, nb);
  const rp_cont_room room = rp_cont_room_for(level, n, depth, levels, max_sync, s->rows.n);
  uint64_t C = room.C, CB = room.CB;
  const uint64_t kcap = room.kcap;
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
  TRY(frame_cont(g, at, &co, out_bin, out_len));
  *done = 1;
  return DG_OK;
}

/* dgr_merkle_continue behind its version check, the next continuation framed `at` bytes into
 * the engine's byte buffer */
static int continue_at(dgr_state* s, uint64_t at, const uint8_t* bin, uint64_t len, uint32_t levels,
                       uint64_t max_sync, int* status, const uint8_t** out_bin, uint64_t* out_len,
                       const uint64_t** keys, uint64_t* n_keys) {
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
  TRY(continue_small(s, at, level, n, nb, levels, max_sync, status, out_bin, out_len, keys, n_keys, &done));
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
    return cont_to_bytes(g, at, &g->co, out_bin, out_len);
  }
  /* {:ok, keys}: the first max_sync_size differing keys (Enum.take, :105) */
  TRY(ri_grow(g, &g->h_ckeys, NULL, &g->h_ckeys_cap, umax(nk, 1)));
  TRY(dg_copy_async(g->e, g->h_ckeys, g->d_ckeys, nk * 8));
  TRY(dg_engine_sync(g->e));
  *keys = g->h_ckeys;
  *n_keys = nk;
  return DG_OK;
}

int dgr_merkle_continue(dgr_state* s, uint64_t version, const uint8_t* bin, uint64_t len, uint32_t levels,
                        uint64_t max_sync, int* status, const uint8_t** out_bin, uint64_t* out_len,
                        const uint64_t** keys, uint64_t* n_keys) {
  if (!s || !bin || !status || !out_bin || !out_len || !keys || !n_keys || !s->has_tree || len < RP_CONT_HEAD)
    return DG_E_INVAL;
  TRY(check_version(s, version));
  return continue_at(s, 0, bin, len, levels, max_sync, status, out_bin, out_len, keys, n_keys);
}

/* One dg_merkle_continues call over the hops `idx[0, m)`: hop idx[i]'s input where it was
 * unpacked (h_msg + moff), its outputs in room[i] at off[i] of `block`. */
typedef struct batch_hop {
  uint32_t level;
  uint64_t n, nb, moff; /* the continuation; its words in h_msg */
  int general;          /* answered by the general calls */
  int64_t bin_at, keys_at; /* byte offsets in h_bin (-1: none) */
} batch_hop;

static int continue_hops(dgr_state* s, const batch_hop* bh, const int* idx, int m, uint64_t* block,
                         const rp_cont_room* room, const uint64_t* off, uint32_t levels, uint64_t max_sync,
                         dg_merkle_cont* cin, dg_merkle_cont* cout, dg_cont_hop* hops, dg_cont_take* const* takes) {
  dgr_engine* g = s->g;
  for (int i = 0; i < m; i++) {
    const batch_hop* b = &bh[idx[i]];
    cin[i] = rp_cont_at(g->h_msg + b->moff, b->level, b->n, b->nb);
    cout[i] = rp_cont_room_out(block, off[i], room[i]);
    memset(&hops[i], 0, sizeof hops[i]);
    hops[i].in = &cin[i];
    hops[i].out = &cout[i];
    hops[i].keys = room[i].kcap ? rp_cont_room_keys(block, off[i], room[i]) : NULL;
    hops[i].cap = room[i].kcap;
  }
  return dg_merkle_continues_take(g->e, &s->tree, &s->rows, m, hops, takes, levels, max_sync);
}

/* A lone leaf-form hop that wants rows: 1 = through the take launch at k = 1, 0 = the single hop
 * and then the take.  DGR_TAKE_LONE=0 / 1 overrides the default (A/B). */
#define TAKE_LONE_DEFAULT 0
static int take_lone(void) {
  static int lone = -1;
  if (lone < 0) {
    const char* v = getenv("DGR_TAKE_LONE");
    lone = v ? atoi(v) != 0 : TAKE_LONE_DEFAULT;
  }
  return lone;
}

/* dgr_merkle_continue_batch (want == NULL), and dgr_merkle_continue_take_batch's answers with the
 * rows that came out of the launch: taken[j].offs != NULL where hop j's did */
static int continue_batch(dgr_state* s, uint64_t version, int k, const uint8_t* const* bins, const uint64_t* lens,
                          const uint8_t* want, uint32_t levels, uint64_t max_sync, dgr_cont_result* results,
                          dgr_hop_rows* taken) {
  if (!s || k < 0 || k > DG_CONT_BATCH_MAX || (k && (!bins || !lens || !results)) || levels < 1) return DG_E_INVAL;
  for (int j = 0; j < k; j++)
    if (!bins[j]) return DG_E_INVAL;
  if (!s->has_tree) return DG_E_INVAL;
  TRY(check_version(s, version));
  if (k == 0) return DG_OK;
  dgr_engine* g = s->g;
  const uint32_t depth = s->tree.depth;
  batch_hop bh[DG_CONT_BATCH_MAX];
  int idx[DG_CONT_BATCH_MAX], m = 0; /* the hops of the launch */
  rp_cont_room room[DG_CONT_BATCH_MAX];
  uint64_t off[DG_CONT_BATCH_MAX + 1], words = 0;
  memset(results, 0, (size_t)k * sizeof *results);
  for (int j = 0; j < k; j++) {
    batch_hop* b = &bh[j];
    memset(b, 0, sizeof *b);
    b->bin_at = b->keys_at = -1;
    results[j].rc = lens[j] < RP_CONT_HEAD ? DG_E_INVAL : rp_cont_parse(bins[j], lens[j], &b->level, &b->n, &b->nb);
    if (results[j].rc != DG_OK) continue;
    const rp_cont_room r = rp_cont_room_for(b->level, b->n, depth, levels, max_sync, s->rows.n);
    b->general = cont_general() || b->n > DG_CONT_HOME_ENTRIES || b->nb > DG_CONT_HOME_BUCKETS ||
                 b->level > depth + 1 || r.C > CONT_SMALL_OUT;
    if (b->general) continue;
    b->moff = words;
    words += even(2 * b->n + b->nb);
    room[m] = r;
    idx[m++] = j;
  }
  /* one hop for the launch: the single call's own launch is 5-6 us shorter (bench_hops); a lone leaf
   * form whose rows are wanted goes the way take_lone() says (bench_hop_take) */
  if (m == 1 && !(take_lone() && want && want[idx[0]] && bh[idx[0]].level == depth + 1)) {
    bh[idx[0]].general = 1;
    m = 0;
  }
  dg_merkle_cont cin[DG_CONT_BATCH_MAX], cout[DG_CONT_BATCH_MAX];
  dg_cont_hop hops[DG_CONT_BATCH_MAX];
  uint64_t at = 0; /* bytes of h_bin in use */
  if (m) {
    /* the m continuations as one message: pos | hash | bucket each, where the kernel reads them */
    TRY(ri_grow_msg(g, words + 1));
    for (int i = 0; i < m; i++) {
      const batch_hop* b = &bh[idx[i]];
      if (2 * b->n + b->nb) memcpy(g->h_msg + b->moff, bins[idx[i]] + RP_CONT_HEAD, (2 * b->n + b->nb) * 8);
    }
    TRY(ri_grow(g, &g->h_bstage, NULL, &g->h_bstage_cap, umax(rp_cont_carve(m, room, off), 1)));
    /* the rows of the leaf forms that want them, out of the same launch */
    dg_cont_take take[DG_CONT_BATCH_MAX];
    dg_cont_take* takes[DG_CONT_BATCH_MAX];
    int n_takes = 0;
    for (int i = 0; i < m; i++) takes[i] = NULL;
    if (want) {
      rp_take_room troom[DG_CONT_BATCH_MAX];
      uint64_t toff[DG_CONT_BATCH_MAX + 1];
      for (int i = 0; i < m; i++) {
        const int on = want[idx[i]] && bh[idx[i]].level == depth + 1;
        troom[i] = rp_take_room_for(on ? room[i].kcap : 0, on ? s->rows.n : 0);
        n_takes += on;
      }
      if (n_takes) TRY(ri_grow(g, &g->h_tstage, NULL, &g->h_tstage_cap, umax(rp_take_carve(m, troom, toff), 1)));
      for (int i = 0; i < m; i++) {
        if (!(want[idx[i]] && bh[idx[i]].level == depth + 1)) continue;
        memset(&take[i], 0, sizeof take[i]);
        take[i].rows = rp_take_room_rows(g->h_tstage, toff[i], troom[i]);
        take[i].offs = rp_take_room_offs(g->h_tstage, toff[i], troom[i]);
        takes[i] = &take[i];
      }
    }
    TRY(continue_hops(s, bh, idx, m, g->h_bstage, room, off, levels, max_sync, cin, cout, hops,
                      n_takes ? takes : NULL));
    /* DG_E_CAPACITY: one retry at the sizes reported, with only the hops that reported it (their
     * outputs staged where a single hop's are: a node form's answer has no keys) */
    int ridx[DG_CONT_BATCH_MAX], rpos[DG_CONT_BATCH_MAX], rm = 0;
    rp_cont_room rroom[DG_CONT_BATCH_MAX];
    for (int i = 0; i < m; i++) {
      if (hops[i].rc != DG_E_CAPACITY) continue;
      const rp_cont_room r = {umax(cout[i].n, room[i].C), umax(cout[i].n_buckets, room[i].CB), 0};
      if (r.C > CONT_SMALL_OUT) {
        bh[idx[i]].general = 1;
        continue;
      }
      rroom[rm] = r;
      rpos[rm] = i;
      ridx[rm++] = idx[i];
    }
    if (rm) {
      dg_merkle_cont rin[DG_CONT_BATCH_MAX], rout[DG_CONT_BATCH_MAX];
      dg_cont_hop rhops[DG_CONT_BATCH_MAX];
      uint64_t roff[DG_CONT_BATCH_MAX + 1];
      TRY(ri_grow(g, &g->h_cstage, NULL, &g->h_cstage_cap, umax(rp_cont_carve(rm, rroom, roff), 1)));
      TRY(continue_hops(s, bh, ridx, rm, g->h_cstage, rroom, roff, levels, max_sync, rin, rout, rhops, NULL));
      for (int i = 0; i < rm; i++) {
        hops[rpos[i]] = rhops[i];
        cout[rpos[i]] = rout[i];
        takes[rpos[i]] = NULL; /* retried without a take (only node forms report capacity) */
      }
    }
    for (int i = 0; i < m; i++) {
      const int j = idx[i];
      if (bh[j].general) continue;
      dgr_cont_result* r = &results[j];
      r->rc = hops[i].rc;
      if (r->rc != DG_OK) continue;
      if (hops[i].status == DG_CONT_DECLINED) {
        bh[j].general = 1;
      } else if (hops[i].status == 0) {
        if (hops[i].n_total > hops[i].n_keys && hops[i].n_keys < max_sync) {
          bh[j].general = 1; /* more keys than kept here */
          continue;
        }
        r->keys = hops[i].keys;
        r->n_keys = hops[i].n_keys;
        if (takes[i] && take[i].rc == DG_OK && r->n_keys) {
          taken[j].rows = take[i].rows;
          taken[j].offs = take[i].offs;
        }
      } else {
        const uint8_t* p;
        r->status = 1;
        r->rc = frame_cont(g, at, &cout[i], &p, &r->len);
        if (r->rc != DG_OK) return r->rc;
        bh[j].bin_at = (int64_t)at;
        at += (r->len + 7) & ~UINT64_C(7);
      }
    }
  }
  /* the rest through the general calls, one by one (they reuse the message buffer and the
   * single hop's staging; what the launch answered is framed by now) */
  for (int j = 0; j < k; j++) {
    if (!bh[j].general) continue;
    dgr_cont_result* r = &results[j];
    const uint8_t* p = NULL;
    const uint64_t* keys = NULL;
    r->rc = continue_at(s, at, bins[j], lens[j], levels, max_sync, &r->status, &p, &r->len, &keys, &r->n_keys);
    if (r->rc != DG_OK) continue;
    if (r->status == 1) {
      bh[j].bin_at = (int64_t)at;
      at += (r->len + 7) & ~UINT64_C(7);
    } else if (r->n_keys) { /* the keys out of the single hop's buffer, which the next hop reuses */
      TRY(bin_room(g, at, r->n_keys * 8));
      memcpy(g->h_bin + at, keys, r->n_keys * 8);
      bh[j].keys_at = (int64_t)at;
      at += r->n_keys * 8;
    }
  }
  for (int j = 0; j < k; j++) { /* (the byte buffer may have moved while it grew) */
    if (bh[j].bin_at >= 0) results[j].bin = g->h_bin + bh[j].bin_at;
    if (bh[j].keys_at >= 0) results[j].keys = (const uint64_t*)(g->h_bin + bh[j].keys_at);
  }
  return DG_OK;
}

int dgr_merkle_continue_batch(dgr_state* s, uint64_t version, int k, const uint8_t* const* bins,
                              const uint64_t* lens, uint32_t levels, uint64_t max_sync, dgr_cont_result* results) {
  return continue_batch(s, version, k, bins, lens, NULL, levels, max_sync, results, NULL);
}

int dgr_merkle_continue_take_batch(dgr_state* s, uint64_t version, int k, const uint8_t* const* bins,
                                   const uint64_t* lens, const uint8_t* want_rows, uint32_t levels,
                                   uint64_t max_sync, dgr_cont_result* results, dgr_hop_rows* taken) {
  if (k > 0 && (!want_rows || !taken)) return DG_E_INVAL;
  if (k > 0 && k <= DG_CONT_BATCH_MAX) memset(taken, 0, (size_t)k * sizeof *taken);
  TRY(continue_batch(s, version, k, bins, lens, want_rows, levels, max_sync, results, taken));
  /* the hops whose rows did not come out of the launch: ONE dgr_take_batch on their keys (host
   * views that it leaves alone), then each hop's rows and offsets laid out on their own */
  const uint64_t* keys[DG_CONT_BATCH_MAX];
  uint64_t nk[DG_CONT_BATCH_MAX];
  int who[DG_CONT_BATCH_MAX], f = 0;
  for (int j = 0; j < k; j++) {
    const dgr_cont_result* r = &results[j];
    if (!want_rows[j] || r->rc != DG_OK || r->status != 0 || !r->n_keys || taken[j].offs) continue;
    keys[f] = r->keys;
    nk[f] = r->n_keys;
    who[f++] = j;
  }
  if (!f) return DG_OK;
  dgr_engine* g = s->g;
  if (f == 1) { /* one hop: dgr_take's keyed gather (no union to sort), its rows as they came home */
    dg_store v;
    TRY(ri_take(s, keys[0], nk[0], &v));
    TRY(ri_grow(g, &g->h_tfall, NULL, &g->h_tfall_cap, nk[0] + 1));
    uint64_t r = 0;
    for (uint64_t i = 0; i < nk[0]; i++) { /* keys and rows ascend together */
      g->h_tfall[i] = r;
      while (r < v.n && v.key[r] == keys[0][i]) r++;
    }
    g->h_tfall[nk[0]] = r;
    if (r != v.n) return DG_E_INVAL;
    taken[who[0]].rows = v;
    taken[who[0]].offs = g->h_tfall;
    return DG_OK;
  }
  dgr_taken u;
  TRY(ri_take_batch(s, f, keys, nk, &u)); /* (the version was checked above, once) */
  uint64_t n[DG_CONT_BATCH_MAX], at[DG_CONT_BATCH_MAX], words = 0;
  for (int i = 0; i < f; i++) {
    n[i] = 0;
    for (uint64_t q = 0; q < u.n_keys; q++)
      if (u.masks[q] >> i & 1) n[i] += u.offs[q + 1] - u.offs[q];
    at[i] = words;
    words += rows_words(n[i]) + even(nk[i] + 1);
  }
  TRY(ri_grow(g, &g->h_tfall, NULL, &g->h_tfall_cap, umax(words, 1)));
  for (int i = 0; i < f; i++) {
    dg_store v = rp_rows(g->h_tfall + at[i], even(n[i]), 0, umax(n[i], 1));
    uint64_t* offs = g->h_tfall + at[i] + rows_words(n[i]);
    uint64_t t = 0;
    for (uint64_t q = 0; q < u.n_keys; q++) { /* the union is ascending, as the hop's keys are */
      if (!(u.masks[q] >> i & 1)) continue;
      const uint64_t a = u.offs[q], c = u.offs[q + 1] - a;
      offs[t++] = v.n;
      memcpy(v.key + v.n, u.rows.key + a, c * 8);
      memcpy(v.val + v.n, u.rows.val + a, c * 8);
      memcpy(v.ts + v.n, u.rows.ts + a, c * 8);
      memcpy(v.node + v.n, u.rows.node + a, c * 4);
      memcpy(v.cnt + v.n, u.rows.cnt + a, c * 8);
      v.n += c;
    }
    offs[t] = v.n;
    if (t != nk[i]) return DG_E_INVAL; /* (a key list that was not ascending and unique) */
    taken[who[i]].rows = v;
    taken[who[i]].offs = offs;
  }
  return DG_OK;
}
