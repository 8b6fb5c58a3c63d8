/*
 * deltagpu_nif.c — the Erlang NIF that binds DeltaCrdt.AWLWWMap (reference
 * lib/delta_crdt/aw_lww_map.ex) and the MerkleMap role of DeltaCrdt.CausalCrdt
 * (lib/delta_crdt/causal_crdt.ex) to libdeltagpu (include/deltagpu.h).  Built by the
 * Elixir project against its OTP's erl_nif.h; this image has no
 * Erlang/OTP, so this file is not compiled here.  The term-independent half
 * (c_src/marshal.c: interning tables, host rows, unmarshal order) is, and is tested
 * from C with the same C-ABI calls this file makes (c_src/test_marshal.c).
 *
 * Resources
 *   engine   a dgr_engine (c_src/replica.h: one dg_engine, one HIP stream, engine-owned
 *            buffers) + the interning universe of this BEAM node + a mutex: every NIF
 *            below takes it (an engine is not re-entrant, and several CausalCrdt
 *            processes call in from several dirty schedulers).
 *   state    a DEVICE-RESIDENT replica state (a dgr_state: rows, context, spare buffer,
 *            tree) at a VERSION.  The Elixir struct keeps `dots` and `value` as real terms
 *            -- CausalCrdt reads them directly (causal_crdt.ex:118,259,331,346) -- and
 *            carries {state, version, pending} beside them; the device answers only the
 *            struct whose version it holds.
 *
 * This file is the term layer only: everything on the device is c_src/replica.c, which
 * the Python mirror of this NIF (delta_crdt_ex_amd/nif.py) and c_src/bench_mutate.c call
 * too.
 *
 * NIFs (dirty-CPU scheduled but resolve_keys; errors are {:error, :stale} for an older
 * struct and {:error, {code, message}} otherwise -- the Elixir side then uses the terms):
 *   engine_open(device)                                -> {:ok, engine}
 *   state_load(engine, dots, value)                    -> {:ok, state, version}
 *   join_delta(state, version, dots, value, keys)      -> {:ok, version', new_dots, changed}
 *        join/3 (aw_lww_map.ex:153-158) of the resident state with a delta
 *        %{dots: dots, value: value} over `keys`, in place on the device
 *        (dg_join_delta_rows); changed = [{key, value_map | nil}] for the keys whose raw
 *        value maps changed (causal_crdt.ex:344-352); the Merkle tree, if built, gets
 *        put/delete + update_hashes of them (:390-394).
 *   mutate_batch(state, version, node, ops)            -> {:ok, version', new_dots, changed}
 *        a batch of {:add, key, value, ts} / {:remove, key} ops by `node` as ONE delta
 *        (dg_mutate_batch, aw_lww_map.ex:99-146) applied like join_delta with the
 *        touched keys (the queued mutations of a GPU-attached replica)
 *   join_deltas(state, version, [{dots, value, keys}])  -> {:ok, version', new_dots, changed}
 *   join_deltas_diffs(state, version, [{dots, value, keys}])
 *                                                      -> {:ok, version', new_dots, changed, diffs}
 *        the pending {:diff, delta, keys} messages of the mailbox joined in one call
 *        (dg_join_deltas); changed and diffs are NET over the batch
 *   sync_from(dst, dst_version, src, src_version, max)  -> {:ok, version', new_dots, changed, n_total}
 *   sync_from_diffs(dst, dst_version, src, src_version, max)
 *                                                      -> {:ok, version', new_dots, changed, n_total, diffs}
 *        one anti-entropy exchange from `src` toward `dst`, two states of ONE engine, device to
 *        device (dgr_sync_from: dg_merkle_diff_take, then the join of the rows where they
 *        stand); n_total the untruncated number of differing keys
 *   read(state, version, keys | :all)                 -> {:ok, %{key => value}}  (:211-224)
 *   take(state, version, keys)                         -> {:ok, value map}  (Map.take, :118,331)
 *   take_batch(state, version, [keys, ...])            -> {:ok, [value map, ...]}  (k takes, one pass)
 *   merkle_build(state, version, depth)                -> :ok
 *   merkle_prepare(state, version, levels)             -> {:continue, cont}     (:255)
 *   merkle_continue(state, version, cont, levels, max) -> {:continue, cont} | {:ok, keys}
 *   merkle_continue_batch(state, version, [cont, ...], levels, max)
 *                                                      -> {:ok, [{:continue, cont} | {:ok, keys}, ...]}
 *        (:96-105; `max` is max_sync_size or :infinite, :98,105,206-214; a key this node
 *        never interned comes back as {:"$dg_key", id})
 *   merkle_continue_take_batch(state, version, [cont, ...], [want, ...], levels, max)
 *                                                      -> {:ok, [{:continue, cont} | {:ok, keys}
 *                                                                | {:ok, keys, value_map}, ...]}
 *        (merkle_continue_batch with Map.take(value, keys), :324-335, where `want` is true)
 *   resolve_keys(engine, keys)                         -> keys (placeholders -> terms)
 *   (a continuation is an opaque binary)
 */
#include <erl_nif.h>
#include <stdlib.h>
#include <string.h>

#include "../include/deltagpu.h"
#include "marshal.h"
#include "replica.h"

/* ------------------------------------------------------------ term operations */
/* Exact map-key order (the order a flatmap's {value, ts} keys are sorted in, which decides
 * read/1's tie-break, aw_lww_map.ex:211-216): the standard term order
 * number < atom < reference < fun < port < pid < tuple < map < list < bitstring, except
 * that numbers compare as map keys do -- every integer before every float ("in maps key
 * order integers types are considered less than floats types") -- recursively inside
 * tuples, lists and maps.  Leaves of one class other than numbers compare by enif_compare
 * (exact and arithmetic order agree there). */
static int term_rank(ErlNifEnv* env, ERL_NIF_TERM t) {
  switch (enif_term_type(env, t)) {
    case ERL_NIF_TERM_TYPE_INTEGER:
    case ERL_NIF_TERM_TYPE_FLOAT: return 0;
    case ERL_NIF_TERM_TYPE_ATOM: return 1;
    case ERL_NIF_TERM_TYPE_REFERENCE: return 2;
    case ERL_NIF_TERM_TYPE_FUN: return 3;
    case ERL_NIF_TERM_TYPE_PORT: return 4;
    case ERL_NIF_TERM_TYPE_PID: return 5;
    case ERL_NIF_TERM_TYPE_TUPLE: return 6;
    case ERL_NIF_TERM_TYPE_MAP: return 7;
    case ERL_NIF_TERM_TYPE_LIST: return 8;
    default: return 9; /* bitstring */
  }
}

static int sgn(int x) { return x < 0 ? -1 : x > 0; }
static int exact_cmp(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b);

/* a map's keys in map-key order (insertion sort: value maps are small) */
static ERL_NIF_TERM* sorted_keys(ErlNifEnv* env, ERL_NIF_TERM m, size_t n) {
  ERL_NIF_TERM* k = (ERL_NIF_TERM*)enif_alloc((n ? n : 1) * sizeof *k);
  ErlNifMapIterator it;
  ERL_NIF_TERM key, val;
  size_t i = 0;
  enif_map_iterator_create(env, m, &it, ERL_NIF_MAP_ITERATOR_FIRST);
  for (; i < n && enif_map_iterator_get_pair(env, &it, &key, &val); enif_map_iterator_next(env, &it)) {
    size_t j = i++;
    for (; j > 0 && exact_cmp(env, k[j - 1], key) > 0; j--) k[j] = k[j - 1];
    k[j] = key;
  }
  enif_map_iterator_destroy(env, &it);
  return k;
}

static int exact_cmp(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b) {
  const int ra = term_rank(env, a), rb = term_rank(env, b);
  if (ra != rb) return ra < rb ? -1 : 1;
  switch (ra) {
    case 0: {
      const int ia = enif_term_type(env, a) == ERL_NIF_TERM_TYPE_INTEGER;
      const int ib = enif_term_type(env, b) == ERL_NIF_TERM_TYPE_INTEGER;
      if (ia != ib) return ia ? -1 : 1;
      return sgn(enif_compare(a, b));
    }
    case 6: {
      int na, nb;
      const ERL_NIF_TERM *ea, *eb;
      enif_get_tuple(env, a, &na, &ea);
      enif_get_tuple(env, b, &nb, &eb);
      if (na != nb) return na < nb ? -1 : 1;
      for (int i = 0; i < na; i++) {
        const int x = exact_cmp(env, ea[i], eb[i]);
        if (x) return x;
      }
      return 0;
    }
    case 7: { /* size, then keys in key order, then values in key order */
      size_t na, nb;
      enif_get_map_size(env, a, &na);
      enif_get_map_size(env, b, &nb);
      if (na != nb) return na < nb ? -1 : 1;
      ERL_NIF_TERM *ka = sorted_keys(env, a, na), *kb = sorted_keys(env, b, nb);
      int x = 0;
      for (size_t i = 0; !x && i < na; i++) x = exact_cmp(env, ka[i], kb[i]);
      for (size_t i = 0; !x && i < na; i++) {
        ERL_NIF_TERM va, vb;
        enif_get_map_value(env, a, ka[i], &va);
        enif_get_map_value(env, b, kb[i], &vb);
        x = exact_cmp(env, va, vb);
      }
      enif_free(ka);
      enif_free(kb);
      return x;
    }
    case 8: /* element-wise, [] first; an improper tail compares as a term */
      for (;;) {
        const int ea = enif_is_empty_list(env, a), eb = enif_is_empty_list(env, b);
        if (ea || eb) return (ea && eb) ? 0 : (ea ? -1 : 1);
        ERL_NIF_TERM ha, ta, hb, tb;
        if (!enif_get_list_cell(env, a, &ha, &ta) || !enif_get_list_cell(env, b, &hb, &tb))
          return exact_cmp(env, a, b); /* a tail that is not a list: of another class */
        const int x = exact_cmp(env, ha, hb);
        if (x) return x;
        a = ta;
        b = tb;
      }
    default:
      return sgn(enif_compare(a, b));
  }
}

typedef struct {
  ErlNifEnv* env; /* the universe's own env: retained terms live here */
} term_ud;

typedef struct {
  ERL_NIF_TERM t;
} boxed;

static int op_cmp(const void* a, const void* b, void* ud) {
  term_ud* u = (term_ud*)ud;
  return exact_cmp(u->env, ((const boxed*)a)->t, ((const boxed*)b)->t);
}

/* The canonical encoding of a term (marshal.h; the Python mirror's interning.canon):
 * key ids, and the node / value term hashes of Merkle rows, are xxh64 of it, so they are
 * the same on every node.  Big integers come from the external term format's digits. */
static int encode_term(ErlNifEnv* env, ERL_NIF_TERM t, dgm_buf* b) {
  switch (enif_term_type(env, t)) {
    case ERL_NIF_TERM_TYPE_INTEGER: {
      ErlNifSInt64 i;
      ErlNifUInt64 u;
      if (enif_get_int64(env, t, &i)) return dgm_enc_i64(b, i);
      if (enif_get_uint64(env, t, &u)) return dgm_enc_u64(b, u);
      ErlNifBinary e; /* SMALL_BIG_EXT 110: n, sign, n digits LE; LARGE_BIG_EXT 111: u32 n */
      if (!enif_term_to_binary(env, t, &e)) return DG_E_NOMEM;
      int rc = DG_E_INVAL;
      if (e.size > 3 && e.data[1] == 110)
        rc = dgm_enc_int(b, e.data[3], e.data + 4, e.data[2]);
      else if (e.size > 6 && e.data[1] == 111)
        rc = dgm_enc_int(b, e.data[6], e.data + 7,
                         ((size_t)e.data[2] << 24) | ((size_t)e.data[3] << 16) | ((size_t)e.data[4] << 8) | e.data[5]);
      enif_release_binary(&e);
      return rc;
    }
    case ERL_NIF_TERM_TYPE_FLOAT: {
      double d;
      enif_get_double(env, t, &d);
      return dgm_enc_float(b, d);
    }
    case ERL_NIF_TERM_TYPE_ATOM: {
      unsigned len;
      if (!enif_get_atom_length(env, t, &len, ERL_NIF_UTF8)) return DG_E_INVAL;
      char* s = (char*)enif_alloc(len + 1);
      enif_get_atom(env, t, s, len + 1, ERL_NIF_UTF8);
      const int rc = dgm_enc_atom(b, s, len);
      enif_free(s);
      return rc;
    }
    case ERL_NIF_TERM_TYPE_BITSTRING: {
      ErlNifBinary bin;
      if (!enif_inspect_binary(env, t, &bin)) return DG_E_INVAL; /* not byte-aligned */
      return dgm_enc_binary(b, bin.data, bin.size);
    }
    case ERL_NIF_TERM_TYPE_TUPLE: {
      int n;
      const ERL_NIF_TERM* e;
      enif_get_tuple(env, t, &n, &e);
      int rc = dgm_enc_tuple(b, (uint32_t)n);
      for (int i = 0; !rc && i < n; i++) rc = encode_term(env, e[i], b);
      return rc;
    }
    case ERL_NIF_TERM_TYPE_LIST: {
      unsigned n;
      if (!enif_get_list_length(env, t, &n)) return DG_E_INVAL; /* improper: unsupported */
      int rc = dgm_enc_list(b, n);
      ERL_NIF_TERM h;
      while (!rc && enif_get_list_cell(env, t, &h, &t)) rc = encode_term(env, h, b);
      return rc;
    }
    case ERL_NIF_TERM_TYPE_MAP: {
      size_t n;
      enif_get_map_size(env, t, &n);
      ERL_NIF_TERM* k = sorted_keys(env, t, n);
      int rc = dgm_enc_map(b, (uint32_t)n);
      for (size_t i = 0; !rc && i < n; i++) {
        ERL_NIF_TERM v;
        enif_get_map_value(env, t, k[i], &v);
        rc = encode_term(env, k[i], b);
        if (!rc) rc = encode_term(env, v, b);
      }
      enif_free(k);
      return rc;
    }
    default: /* pids, ports, references, funs: node-local terms, not interned */
      return DG_E_INVAL;
  }
}

static int op_encode(const void* p, dgm_buf* b, void* ud) {
  term_ud* u = (term_ud*)ud;
  return encode_term(u->env, ((const boxed*)p)->t, b);
}

static void* op_keep(const void* p, void* ud) {
  term_ud* u = (term_ud*)ud;
  boxed* c = (boxed*)enif_alloc(sizeof *c);
  c->t = enif_make_copy(u->env, ((const boxed*)p)->t);
  return c;
}

static void op_drop(void* p, void* ud) {
  (void)ud;
  enif_free(p);
}

/* ------------------------------------------------------------ resources */
typedef struct {
  dgr_engine* r;   /* the device half: states, buffers, term tables (c_src/replica.h) */
  dgm_universe* u; /* the interning tables of this BEAM node */
  term_ud tu;
  ErlNifMutex* lock;
} engine_res;

typedef struct {
  engine_res* eng;
  dgr_state* s; /* the device-resident state; its version is in every struct that holds it */
} state_res;

static ErlNifResourceType* ENGINE_RT;
static ErlNifResourceType* STATE_RT;
static ERL_NIF_TERM A_OK, A_ERROR, A_NIL, A_ALL, A_CONTINUE, A_MAP, A_STRUCT, A_MAPSET, A_STALE,
    A_INFINITE, A_DGKEY, A_ADD, A_REMOVE;

static void engine_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  engine_res* r = (engine_res*)obj;
  if (r->r) dgr_engine_close(r->r); /* every state resource holds the engine: none is left */
  if (r->u) dgm_universe_free(r->u);
  if (r->tu.env) enif_free_env(r->tu.env);
  if (r->lock) enif_mutex_destroy(r->lock);
}

static void state_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  state_res* s = (state_res*)obj;
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  dgr_state_free(s->s);
  enif_mutex_unlock(g->lock);
  enif_release_resource(g);
}

/* {:error, :stale} for an older struct (its terms are authoritative: the Elixir side reads
 * or joins those on the CPU), {:error, {code, message}} otherwise */
static ERL_NIF_TERM error_term(ErlNifEnv* env, int rc) {
  if (rc == DGR_E_STALE) return enif_make_tuple2(env, A_ERROR, A_STALE);
  return enif_make_tuple2(env, A_ERROR,
                          enif_make_tuple2(env, enif_make_int(env, rc),
                                           enif_make_string(env, dg_last_error(), ERL_NIF_LATIN1)));
}

#define TRY(x)                          \
  do {                                  \
    int rc_ = (x);                      \
    if (rc_ != DG_OK) { rc = rc_; goto out; } \
  } while (0)

/* ------------------------------------------------------------ marshal */
/* The universe's term-hash tables to the device (when they grew or a relabel changed the
 * value ids); every tree of the engine hashes rows through them. */
static int refresh_terms(engine_res* g) {
  const uint64_t *nh, *vid, *vh;
  uint32_t nn;
  uint64_t nv;
  dgm_node_hashes(g->u, &nh, &nn);
  dgm_value_hashes(g->u, &vid, &vh, &nv);
  return dgr_refresh_terms(g->r, nh, nn, vid, vh, nv);
}

/* After any dgm_value that relabelled: every live state's val column rewritten
 * (dgr_remap).  Trees hash terms, so they stay valid; versions do not move. */
static int remap_live(engine_res* g) {
  const uint64_t *old_ids, *new_ids;
  uint64_t n;
  dgm_last_relabel(g->u, &old_ids, &new_ids, &n);
  return dgr_remap(g->r, old_ids, new_ids, n);
}

static int intern_value(ErlNifEnv* env, engine_res* g, ERL_NIF_TERM v, uint64_t* id) {
  boxed b = {v};
  (void)env;
  int relabeled = 0;
  int rc = dgm_value(g->u, &b, id, &relabeled);
  if (!rc && relabeled) rc = remap_live(g);
  return rc;
}

/* a MapSet's members: %MapSet{map: %{member => []}} (Elixir 1.7+) */
static int mapset_map(ErlNifEnv* env, ERL_NIF_TERM set, ERL_NIF_TERM* map) {
  return enif_get_map_value(env, set, A_MAP, map);
}

/* every value of %{key => %{{v, ts} => dots}} interned (a relabel re-spaces ids already handed
 * out, so this runs before any row that holds an id is written: for a batch of deltas, over
 * every delta before the first one's rows) */
static int intern_values(ErlNifEnv* env, engine_res* g, ERL_NIF_TERM value) {
  ErlNifMapIterator ki, ei;
  ERL_NIF_TERM key, entries, vt, dots;
  if (!enif_map_iterator_create(env, value, &ki, ERL_NIF_MAP_ITERATOR_FIRST)) return DG_E_INVAL;
  for (; enif_map_iterator_get_pair(env, &ki, &key, &entries); enif_map_iterator_next(env, &ki)) {
    if (!enif_map_iterator_create(env, entries, &ei, ERL_NIF_MAP_ITERATOR_FIRST)) return DG_E_INVAL;
    for (; enif_map_iterator_get_pair(env, &ei, &vt, &dots); enif_map_iterator_next(env, &ei)) {
      int ar;
      const ERL_NIF_TERM* e;
      uint64_t id;
      if (!enif_get_tuple(env, vt, &ar, &e) || ar != 2 || intern_value(env, g, e[0], &id)) {
        enif_map_iterator_destroy(env, &ei);
        enif_map_iterator_destroy(env, &ki);
        return DG_E_INVAL;
      }
    }
    enif_map_iterator_destroy(env, &ei);
  }
  enif_map_iterator_destroy(env, &ki);
  return DG_OK;
}

/* walk %{key => %{{v, ts} => MapSet[{node, counter}]}} in map order into host rows */
static int marshal_value(ErlNifEnv* env, engine_res* g, ERL_NIF_TERM value, dgm_rows* out) {
  ErlNifMapIterator ki, ei, di;
  ERL_NIF_TERM key, entries, vt, dots, dmap, dot, unused;
  /* pass 1: intern every value first */
  const int rc1 = intern_values(env, g, value);
  if (rc1) return rc1;
  /* pass 2: the rows */
  enif_map_iterator_create(env, value, &ki, ERL_NIF_MAP_ITERATOR_FIRST);
  for (; enif_map_iterator_get_pair(env, &ki, &key, &entries); enif_map_iterator_next(env, &ki)) {
    boxed bk = {key};
    uint64_t kid;
    if (dgm_key(g->u, &bk, &kid)) goto bad_k;
    enif_map_iterator_create(env, entries, &ei, ERL_NIF_MAP_ITERATOR_FIRST);
    for (; enif_map_iterator_get_pair(env, &ei, &vt, &dots); enif_map_iterator_next(env, &ei)) {
      int ar;
      const ERL_NIF_TERM* e;
      ErlNifSInt64 ts;
      uint64_t vid;
      int rl = 0;
      boxed bv;
      enif_get_tuple(env, vt, &ar, &e);
      bv.t = e[0];
      if (dgm_value(g->u, &bv, &vid, &rl) || rl || !enif_get_int64(env, e[1], &ts) ||
          !mapset_map(env, dots, &dmap) ||
          !enif_map_iterator_create(env, dmap, &di, ERL_NIF_MAP_ITERATOR_FIRST))
        goto bad_e;
      for (; enif_map_iterator_get_pair(env, &di, &dot, &unused); enif_map_iterator_next(env, &di)) {
        const ERL_NIF_TERM* d;
        ErlNifUInt64 cnt;
        uint32_t nid;
        boxed bn;
        if (!enif_get_tuple(env, dot, &ar, &d) || ar != 2 || !enif_get_uint64(env, d[1], &cnt)) goto bad_d;
        bn.t = d[0];
        if (dgm_node(g->u, &bn, &nid) || dgm_rows_push(out, kid, vid, ts, nid, cnt)) goto bad_d;
      }
      enif_map_iterator_destroy(env, &di);
    }
    enif_map_iterator_destroy(env, &ei);
  }
  enif_map_iterator_destroy(env, &ki);
  return DG_OK;
bad_d:
  enif_map_iterator_destroy(env, &di);
bad_e:
  enif_map_iterator_destroy(env, &ei);
bad_k:
  enif_map_iterator_destroy(env, &ki);
  return DG_E_INVAL;
}

/* a context: a MapSet of dots (DG_CTX_DOTS) or a %{node => max} VV (DG_CTX_VV) */
static int marshal_dots(ErlNifEnv* env, engine_res* g, ERL_NIF_TERM dots, dgm_rows* out) {
  ERL_NIF_TERM m, k, v, st;
  const int is_set = enif_get_map_value(env, dots, A_STRUCT, &st) && enif_is_identical(st, A_MAPSET);
  out->c.kind = is_set ? DG_CTX_DOTS : DG_CTX_VV;
  if (is_set) {
    if (!mapset_map(env, dots, &m)) return DG_E_INVAL;
  } else {
    m = dots;
  }
  ErlNifMapIterator it;
  if (!enif_map_iterator_create(env, m, &it, ERL_NIF_MAP_ITERATOR_FIRST)) return DG_E_INVAL;
  for (; enif_map_iterator_get_pair(env, &it, &k, &v); enif_map_iterator_next(env, &it)) {
    ERL_NIF_TERM node = k, cnt_t = v;
    int ar;
    const ERL_NIF_TERM* d;
    if (is_set) {
      if (!enif_get_tuple(env, k, &ar, &d) || ar != 2) goto bad;
      node = d[0];
      cnt_t = d[1];
    }
    ErlNifUInt64 cnt;
    uint32_t nid;
    boxed bn = {node};
    if (!enif_get_uint64(env, cnt_t, &cnt) || dgm_node(g->u, &bn, &nid) || dgm_ctx_push(out, nid, cnt))
      goto bad;
  }
  enif_map_iterator_destroy(env, &it);
  return DG_OK;
bad:
  enif_map_iterator_destroy(env, &it);
  return DG_E_INVAL;
}

/* {:"$dg_key", id}: a differing key this node never interned (only the peer holds it),
 * named by its id -- merkle_continue's {:ok, keys} holds such placeholders, every NIF
 * that takes keys accepts them as the id, and resolve_keys turns them back into terms on
 * a node that knows the key (the originator's get_diff, causal_crdt.ex:112-123). */
static int placeholder_id(ErlNifEnv* env, ERL_NIF_TERM t, uint64_t* id) {
  int ar;
  const ERL_NIF_TERM* e;
  ErlNifUInt64 x;
  if (!enif_get_tuple(env, t, &ar, &e) || ar != 2 || !enif_is_identical(e[0], A_DGKEY) ||
      !enif_get_uint64(env, e[1], &x))
    return 0;
  *id = x;
  return 1;
}

/* a key list -> host key ids (any order; the replica layer sorts them) */
static int marshal_keys(ErlNifEnv* env, engine_res* g, ERL_NIF_TERM keys, uint64_t** ids, uint64_t* n_keys) {
  unsigned len;
  *ids = NULL;
  *n_keys = 0;
  if (!enif_get_list_length(env, keys, &len)) return DG_E_INVAL;
  *ids = (uint64_t*)enif_alloc((len ? len : 1) * sizeof **ids);
  if (!*ids) return DG_E_NOMEM;
  ERL_NIF_TERM h, t = keys;
  unsigned n = 0;
  while (enif_get_list_cell(env, t, &h, &t)) {
    if (placeholder_id(env, h, &(*ids)[n])) {
      n++;
      continue;
    }
    boxed b = {h};
    if (dgm_key(g->u, &b, &(*ids)[n++])) return DG_E_INVAL;
  }
  *n_keys = n;
  return DG_OK;
}

/* the key's term, or {:"$dg_key", id} when this node never interned it */
static ERL_NIF_TERM key_term(ErlNifEnv* env, engine_res* g, uint64_t id) {
  const boxed* b = (const boxed*)dgm_key_term(g->u, id);
  if (b) return enif_make_copy(env, b->t);
  return enif_make_tuple2(env, A_DGKEY, enif_make_uint64(env, id));
}

/* ------------------------------------------------------------ unmarshal */
typedef struct {
  ErlNifEnv* env;
  engine_res* g;
  ERL_NIF_TERM out;     /* %{key => %{{v, ts} => MapSet}} being built */
  ERL_NIF_TERM entries; /* the current key's map */
  ERL_NIF_TERM dots;    /* the current entry's MapSet map */
  ERL_NIF_TERM key, vt;
  int open_key, open_entry;
} unm;

static ERL_NIF_TERM make_mapset(ErlNifEnv* env, ERL_NIF_TERM map) {
  ERL_NIF_TERM ks[3] = {A_STRUCT, A_MAP, enif_make_atom(env, "version")};
  ERL_NIF_TERM vs[3] = {A_MAPSET, map, enif_make_int(env, 2)};
  ERL_NIF_TERM s;
  enif_make_map_from_arrays(env, ks, vs, 3, &s);
  return s;
}

static void close_entry(unm* u) {
  if (u->open_entry) {
    enif_make_map_put(u->env, u->entries, u->vt, make_mapset(u->env, u->dots), &u->entries);
    u->open_entry = 0;
  }
}
static void close_key(unm* u) {
  close_entry(u);
  if (u->open_key) {
    enif_make_map_put(u->env, u->out, u->key, u->entries, &u->out);
    u->open_key = 0;
  }
}
static int u_key(void* ud, uint64_t key, uint64_t n) {
  (void)n;
  unm* u = (unm*)ud;
  close_key(u);
  const boxed* b = (const boxed*)dgm_key_term(u->g->u, key);
  if (!b) return DG_E_INVAL;
  u->key = enif_make_copy(u->env, b->t);
  u->entries = enif_make_new_map(u->env);
  u->open_key = 1;
  return 0;
}
/* the term of a value id: a canonical integer from its closed form, else the table's */
static int value_term(ErlNifEnv* env, engine_res* g, uint64_t id, ERL_NIF_TERM* out) {
  int64_t v;
  if (dgm_value_is_canonical(id, &v)) {
    *out = enif_make_int64(env, v);
    return DG_OK;
  }
  const boxed* b = (const boxed*)dgm_value_term(g->u, id);
  if (!b) return DG_E_INVAL;
  *out = enif_make_copy(env, b->t);
  return DG_OK;
}

static int u_entry(void* ud, uint64_t val, int64_t ts, uint64_t n) {
  (void)n;
  unm* u = (unm*)ud;
  close_entry(u);
  ERL_NIF_TERM vt;
  if (value_term(u->env, u->g, val, &vt)) return DG_E_INVAL;
  u->vt = enif_make_tuple2(u->env, vt, enif_make_int64(u->env, ts));
  u->dots = enif_make_new_map(u->env);
  u->open_entry = 1;
  return 0;
}
static int u_dot(void* ud, uint32_t node, uint64_t cnt) {
  unm* u = (unm*)ud;
  const boxed* b = (const boxed*)dgm_node_term(u->g->u, node);
  if (!b) return DG_E_INVAL;
  ERL_NIF_TERM d = enif_make_tuple2(u->env, enif_make_copy(u->env, b->t), enif_make_uint64(u->env, cnt));
  enif_make_map_put(u->env, u->dots, d, enif_make_list(u->env, 0), &u->dots);
  return 0;
}

/* host rows -> %{key => value map} */
static int unmarshal_host_rows(ErlNifEnv* env, engine_res* g, const dg_store* h, ERL_NIF_TERM* out) {
  unm u;
  memset(&u, 0, sizeof u);
  u.env = env;
  u.g = g;
  u.out = enif_make_new_map(env);
  dgm_walk w = {u_key, u_entry, u_dot};
  const int rc = dgm_walk_rows(h, &w, &u);
  close_key(&u);
  *out = u.out;
  return rc;
}

/* a host context -> a %{node => max} VV or a MapSet of dots */
static int unmarshal_dots(ErlNifEnv* env, engine_res* g, const dg_context* c, ERL_NIF_TERM* out) {
  ERL_NIF_TERM m = enif_make_new_map(env);
  for (uint64_t i = 0; i < c->n; i++) {
    const boxed* b = (const boxed*)dgm_node_term(g->u, c->node[i]);
    if (!b) return DG_E_INVAL;
    ERL_NIF_TERM n = enif_make_copy(env, b->t), k = enif_make_uint64(env, c->cnt[i]);
    if (c->kind == DG_CTX_VV)
      enif_make_map_put(env, m, n, k, &m);
    else
      enif_make_map_put(env, m, enif_make_tuple2(env, n, k), enif_make_list(env, 0), &m);
  }
  *out = c->kind == DG_CTX_VV ? m : make_mapset(env, m);
  return DG_OK;
}

/* ------------------------------------------------------------ NIFs */
static ERL_NIF_TERM engine_open(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  int dev;
  if (!enif_get_int(env, argv[0], &dev)) return enif_make_badarg(env);
  engine_res* g = (engine_res*)enif_alloc_resource(ENGINE_RT, sizeof *g);
  memset(g, 0, sizeof *g);
  g->lock = enif_mutex_create("deltagpu_engine");
  g->tu.env = enif_alloc_env();
  dgm_term_ops ops = {op_cmp, op_encode, NULL, op_keep, op_drop, &g->tu};
  g->u = dgm_universe_new(&ops);
  const int rc = dgr_engine_open(dev, &g->r);
  ERL_NIF_TERM r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, enif_make_resource(env, g));
  enif_release_resource(g);
  return r;
}

static int get_state(ErlNifEnv* env, ERL_NIF_TERM t, ERL_NIF_TERM v, state_res** s, uint64_t* version) {
  ErlNifUInt64 x;
  if (!enif_get_resource(env, t, STATE_RT, (void**)s) || !enif_get_uint64(env, v, &x)) return 0;
  *version = x;
  return 1;
}

/* state_load(engine, dots, value) -> {:ok, state, version} */
static ERL_NIF_TERM state_load(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  engine_res* g;
  if (!enif_get_resource(env, argv[0], ENGINE_RT, (void**)&g)) return enif_make_badarg(env);
  enif_mutex_lock(g->lock);
  dgm_rows h;
  dgr_state* ds = NULL;
  int rc = dgm_rows_init(&h, 1024, 64);
  ERL_NIF_TERM r;
  if (!rc) rc = marshal_dots(env, g, argv[1], &h);
  if (!rc) rc = marshal_value(env, g, argv[2], &h);
  if (!rc) rc = dgr_state_load(g->r, &h.s, &h.c, &ds);
  dgm_rows_free(&h);
  if (rc) {
    r = error_term(env, rc);
  } else {
    state_res* s = (state_res*)enif_alloc_resource(STATE_RT, sizeof *s);
    enif_keep_resource(g);
    s->eng = g;
    s->s = ds;
    r = enif_make_tuple3(env, A_OK, enif_make_resource(env, s), enif_make_uint64(env, dgr_state_version(ds)));
    enif_release_resource(s);
  }
  enif_mutex_unlock(g->lock);
  return r;
}

/* diffs_to_callback/3's list (causal_crdt.ex:361-381) from the device's reads of the changed
 * keys before and after the join: [{:add, key, value} | {:remove, key}] in ascending key-id
 * order, the order of `changed` (the reference emits them in `keys` order; a consumer must
 * not rely on the order inside one callback list) */
static int diffs_list(ErlNifEnv* env, engine_res* g, const dgr_changed* c, const dgr_diffs* d,
                      ERL_NIF_TERM* out) {
  ERL_NIF_TERM l = enif_make_list(env, 0);
  boxed bn = {A_NIL};
  uint64_t nil_id = 0;
  const int has_nil = dgm_value_find(g->u, &bn, &nil_id);
  if (has_nil < 0) return has_nil;
  uint8_t* kind = (uint8_t*)enif_alloc(d->n ? d->n : 1);
  if (!kind) return DG_E_NOMEM;
  dgm_classify_diffs(d->old_val, d->new_val, d->flags, d->n, has_nil, nil_id, kind);
  int rc = DG_OK;
  for (uint64_t i = d->n; i-- > 0 && !rc;) {
    if (kind[i] == DGM_DIFF_NONE) continue;
    const boxed* b = (const boxed*)dgm_key_term(g->u, c->keys[i]);
    if (!b) {
      rc = DG_E_INVAL;
      break;
    }
    ERL_NIF_TERM k = enif_make_copy(env, b->t), v;
    if (kind[i] == DGM_DIFF_REMOVE) {
      l = enif_make_list_cell(env, enif_make_tuple2(env, A_REMOVE, k), l);
    } else if (!(rc = value_term(env, g, d->new_val[i], &v))) {
      l = enif_make_list_cell(env, enif_make_tuple3(env, A_ADD, k, v), l);
    }
  }
  enif_free(kind);
  *out = l;
  return rc;
}

/* {:ok, version, new_dots, [{key, value_map | nil}]} from a join's result: the changed
 * keys' rows (in key order) walked into value maps, the context into its term; with `d`
 * {:ok, version, new_dots, changed, diffs} */
static int changed_result_total(ErlNifEnv* env, engine_res* g, const dgr_changed* c, const dgr_diffs* d,
                                const uint64_t* n_total, ERL_NIF_TERM* r);
static int changed_result(ErlNifEnv* env, engine_res* g, const dgr_changed* c, const dgr_diffs* d,
                          ERL_NIF_TERM* r) {
  return changed_result_total(env, g, c, d, NULL, r);
}

/* ... with n_total (sync_from): {:ok, version, new_dots, changed, n_total [, diffs]} */
static int changed_result_total(ErlNifEnv* env, engine_res* g, const dgr_changed* c, const dgr_diffs* d,
                                const uint64_t* n_total, ERL_NIF_TERM* r) {
  ERL_NIF_TERM values, dots, changed = enif_make_list(env, 0);
  int rc = unmarshal_host_rows(env, g, &c->rows, &values);
  if (!rc) rc = unmarshal_dots(env, g, &c->ctx, &dots);
  if (rc) return rc;
  for (uint64_t i = c->n_changed; i-- > 0;) {
    const boxed* b = (const boxed*)dgm_key_term(g->u, c->keys[i]);
    if (!b) return DG_E_INVAL;
    ERL_NIF_TERM k = enif_make_copy(env, b->t), v;
    if (!enif_get_map_value(env, values, k, &v)) v = A_NIL; /* the key's entries all went */
    changed = enif_make_list_cell(env, enif_make_tuple2(env, k, v), changed);
  }
  if (d) {
    ERL_NIF_TERM diffs;
    if ((rc = diffs_list(env, g, c, d, &diffs))) return rc;
    *r = n_total ? enif_make_tuple6(env, A_OK, enif_make_uint64(env, c->version), dots, changed,
                                    enif_make_uint64(env, *n_total), diffs)
                 : enif_make_tuple5(env, A_OK, enif_make_uint64(env, c->version), dots, changed, diffs);
    return DG_OK;
  }
  *r = n_total ? enif_make_tuple5(env, A_OK, enif_make_uint64(env, c->version), dots, changed,
                                  enif_make_uint64(env, *n_total))
               : enif_make_tuple4(env, A_OK, enif_make_uint64(env, c->version), dots, changed);
  return DG_OK;
}

/* join_delta(state, version, dots, value, keys) -> {:ok, version', new_dots, changed}
 * join/3 (aw_lww_map.ex:153-158) of the resident state with the delta %{dots, value} over
 * `keys`, in place on the device; `changed` = the keys whose raw value maps changed
 * (causal_crdt.ex:344-352) with their new maps; the tree (if built) gets their put/delete. */
static ERL_NIF_TERM join_delta_impl(ErlNifEnv* env, const ERL_NIF_TERM argv[], int with_diffs) {
  state_res* s;
  uint64_t version;
  if (!get_state(env, argv[0], argv[1], &s, &version)) return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  dgm_rows h;
  uint64_t *keys = NULL, n_keys = 0;
  dgr_changed c;
  ERL_NIF_TERM r = A_NIL;
  TRY(dgm_rows_init(&h, 256, 16));
  TRY(marshal_dots(env, g, argv[2], &h));
  TRY(marshal_value(env, g, argv[3], &h));
  TRY(marshal_keys(env, g, argv[4], &keys, &n_keys));
  if (dgr_state_has_tree(s->s)) TRY(refresh_terms(g));
  if (with_diffs) {
    dgr_diffs d;
    TRY(dgr_join_delta_diffs(s->s, version, &h.s, &h.c, keys, n_keys, &c, &d));
    TRY(changed_result(env, g, &c, &d, &r));
  } else {
    TRY(dgr_join_delta(s->s, version, &h.s, &h.c, keys, n_keys, &c));
    TRY(changed_result(env, g, &c, NULL, &r));
  }
out:
  if (rc) r = error_term(env, rc);
  dgm_rows_free(&h);
  if (keys) enif_free(keys);
  enif_mutex_unlock(g->lock);
  return r;
}

static ERL_NIF_TERM join_delta(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return join_delta_impl(env, argv, 0);
}

/* join_delta_diffs(state, version, dots, value, keys) -> {:ok, version', new_dots, changed,
 * diffs}: join_delta plus what on_diffs receives, from the device's reads of the changed keys
 * before and after the join (dgr_join_delta_diffs) -- no old struct is read */
static ERL_NIF_TERM join_delta_diffs(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return join_delta_impl(env, argv, 1);
}

/* sync_from(dst, dst_version, src, src_version, max_sync_size | :infinite)
 *   -> {:ok, version', new_dots, changed, n_total}
 * One anti-entropy exchange from `src` toward `dst`, two states of ONE engine, device to device
 * (dgr_sync_from): the trees' diff answered with src's rows of the first max_sync_size differing
 * keys, joined into dst where they stand -- no row becomes a term, none is interned again.
 * n_total: the untruncated number of differing keys (another round while it exceeds
 * max_sync_size).  The result marshals exactly as join_delta's; sync_from_diffs appends diffs. */
static ERL_NIF_TERM sync_from_impl(ErlNifEnv* env, const ERL_NIF_TERM argv[], int with_diffs) {
  state_res *s, *src;
  uint64_t version, src_version, n_total = 0;
  ErlNifUInt64 max_sync = 0; /* (dgr_sync_from: 0 is :infinite) */
  if (!get_state(env, argv[0], argv[1], &s, &version) || !get_state(env, argv[2], argv[3], &src, &src_version) ||
      (!enif_is_identical(argv[4], A_INFINITE) && (!enif_get_uint64(env, argv[4], &max_sync) || max_sync == 0)))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  if (src->eng != g) return error_term(env, DG_E_INVAL); /* (one engine, one lock) */
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  dgr_changed c;
  ERL_NIF_TERM r = A_NIL;
  if (dgr_state_has_tree(s->s) && dgr_state_has_tree(src->s)) TRY(refresh_terms(g));
  if (with_diffs) {
    dgr_diffs d;
    TRY(dgr_sync_from_diffs(s->s, version, src->s, src_version, max_sync, &c, &d, &n_total));
    TRY(changed_result_total(env, g, &c, &d, &n_total, &r));
  } else {
    TRY(dgr_sync_from(s->s, version, src->s, src_version, max_sync, &c, &n_total));
    TRY(changed_result_total(env, g, &c, NULL, &n_total, &r));
  }
out:
  if (rc) r = error_term(env, rc);
  enif_mutex_unlock(g->lock);
  return r;
}

static ERL_NIF_TERM sync_from_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return sync_from_impl(env, argv, 0);
}

static ERL_NIF_TERM sync_from_diffs_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return sync_from_impl(env, argv, 1);
}

/* join_deltas(state, version, [{dots, value, keys}, ...]) -> {:ok, version', new_dots, changed}
 * The pending {:diff, delta, keys} messages of a replica's mailbox joined in ONE call
 * (dgr_join_deltas: one packed message, one fold over the state, the diff of the state before
 * and after): `changed` is the batch's NET change, and join_deltas_diffs' `diffs` are net too
 * -- a key is reported once, with its read before the first and after the last delta; the
 * callbacks the reference would have made per delta are not reproduced. */
static ERL_NIF_TERM join_deltas_impl(ErlNifEnv* env, const ERL_NIF_TERM argv[], int with_diffs) {
  state_res* s;
  uint64_t version;
  unsigned k = 0;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_list_length(env, argv[2], &k))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  const unsigned kk = k ? k : 1;
  dgm_rows* h = (dgm_rows*)enif_alloc(kk * sizeof *h);
  dg_store* st = (dg_store*)enif_alloc(kk * sizeof *st);
  dg_context* cx = (dg_context*)enif_alloc(kk * sizeof *cx);
  uint64_t** keys = (uint64_t**)enif_alloc(kk * sizeof *keys);
  uint64_t* n_keys = (uint64_t*)enif_alloc(kk * sizeof *n_keys);
  unsigned n_init = 0;
  dgr_changed c;
  ERL_NIF_TERM r = A_NIL, head, tail;
  if (!h || !st || !cx || !keys || !n_keys) TRY(DG_E_NOMEM);
  for (unsigned i = 0; i < kk; i++) keys[i] = NULL;
  /* every delta's values first, then the rows (intern_values) */
  for (tail = argv[2]; enif_get_list_cell(env, tail, &head, &tail);) {
    int ar;
    const ERL_NIF_TERM* e;
    if (!enif_get_tuple(env, head, &ar, &e) || ar != 3) TRY(DG_E_INVAL);
    TRY(intern_values(env, g, e[1]));
  }
  for (tail = argv[2]; enif_get_list_cell(env, tail, &head, &tail); n_init++) {
    int ar;
    const ERL_NIF_TERM* e;
    enif_get_tuple(env, head, &ar, &e);
    TRY(dgm_rows_init(&h[n_init], 256, 16));
    const unsigned i = n_init;
    rc = marshal_dots(env, g, e[0], &h[i]);
    if (!rc) rc = marshal_value(env, g, e[1], &h[i]);
    if (!rc) rc = marshal_keys(env, g, e[2], &keys[i], &n_keys[i]);
    st[i] = h[i].s;
    cx[i] = h[i].c;
    if (rc) {
      n_init++;
      goto out;
    }
  }
  if (dgr_state_has_tree(s->s)) TRY(refresh_terms(g));
  if (with_diffs) {
    dgr_diffs d;
    TRY(dgr_join_deltas_diffs(s->s, version, (int)k, st, cx, (const uint64_t* const*)keys, n_keys, &c, &d));
    TRY(changed_result(env, g, &c, &d, &r));
  } else {
    TRY(dgr_join_deltas(s->s, version, (int)k, st, cx, (const uint64_t* const*)keys, n_keys, &c));
    TRY(changed_result(env, g, &c, NULL, &r));
  }
out:
  if (rc) r = error_term(env, rc);
  for (unsigned i = 0; i < n_init; i++) dgm_rows_free(&h[i]);
  for (unsigned i = 0; keys && i < kk; i++)
    if (keys[i]) enif_free(keys[i]);
  if (h) enif_free(h);
  if (st) enif_free(st);
  if (cx) enif_free(cx);
  if (keys) enif_free(keys);
  if (n_keys) enif_free(n_keys);
  enif_mutex_unlock(g->lock);
  return r;
}

static ERL_NIF_TERM join_deltas_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return join_deltas_impl(env, argv, 0);
}

static ERL_NIF_TERM join_deltas_diffs_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return join_deltas_impl(env, argv, 1);
}

/* mutate_batch(state, version, node, ops) -> {:ok, version', new_dots, changed}: a batch of
 * mutations by `node` -- ops = [{:add, key, value, ts} | {:remove, key}] in the order they
 * were made (the queued mutations of a GPU-attached replica, causal_crdt.ex:196-198,
 * 337-342) -- as ONE delta built on the device (dg_mutate_batch: per touched key the last
 * op's row if it is an add, context = the touched keys' dots plus every add's dot,
 * aw_lww_map.ex:99-146), applied like join_delta with the touched keys. */
static ERL_NIF_TERM mutate_batch_impl(ErlNifEnv* env, const ERL_NIF_TERM argv[], int with_diffs) {
  state_res* s;
  uint64_t version;
  unsigned m;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_list_length(env, argv[3], &m))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  uint32_t node = 0;
  dgr_changed c;
  ERL_NIF_TERM r = A_NIL, head, tail = argv[3];
  uint8_t* kind = (uint8_t*)enif_alloc(m ? m : 1);
  uint64_t* key = (uint64_t*)enif_alloc((m ? m : 1) * 8);
  uint64_t* val = (uint64_t*)enif_alloc((m ? m : 1) * 8);
  int64_t* ts = (int64_t*)enif_alloc((m ? m : 1) * 8);
  if (!kind || !key || !val || !ts) {
    rc = DG_E_NOMEM;
    goto out;
  }
  {
    boxed bn = {argv[2]};
    TRY(dgm_node(g->u, &bn, &node));
  }
  /* pass 1: every value interned (a relabel re-spaces ids already handed out) */
  for (unsigned i = 0; i < m; i++) {
    int ar;
    const ERL_NIF_TERM* e;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &ar, &e) ||
        (ar != 2 && ar != 4)) {
      rc = DG_E_INVAL;
      goto out;
    }
    kind[i] = ar == 4;
    val[i] = 0;
    ts[i] = 0;
    if (ar == 4) {
      ErlNifSInt64 t;
      if (!enif_get_int64(env, e[3], &t)) {
        rc = DG_E_INVAL;
        goto out;
      }
      ts[i] = t;
      TRY(intern_value(env, g, e[2], &val[i]));
    }
  }
  /* pass 2: keys, and the value ids as they stand after any relabel */
  tail = argv[3];
  for (unsigned i = 0; i < m; i++) {
    int ar;
    const ERL_NIF_TERM* e;
    enif_get_list_cell(env, tail, &head, &tail);
    enif_get_tuple(env, head, &ar, &e);
    boxed bk = {e[1]};
    TRY(dgm_key(g->u, &bk, &key[i]));
    if (ar == 4) {
      boxed bv = {e[2]};
      int relabeled = 0;
      TRY(dgm_value(g->u, &bv, &val[i], &relabeled));
      if (relabeled) TRY(remap_live(g));
    }
  }
  if (dgr_state_has_tree(s->s)) TRY(refresh_terms(g));
  if (with_diffs) {
    dgr_diffs d;
    TRY(dgr_mutate_batch_diffs(s->s, version, node, m, kind, key, val, ts, &c, &d));
    TRY(changed_result(env, g, &c, &d, &r));
  } else {
    TRY(dgr_mutate_batch(s->s, version, node, m, kind, key, val, ts, &c));
    TRY(changed_result(env, g, &c, NULL, &r));
  }
out:
  if (rc) r = error_term(env, rc);
  if (kind) enif_free(kind);
  if (key) enif_free(key);
  if (val) enif_free(val);
  if (ts) enif_free(ts);
  enif_mutex_unlock(g->lock);
  return r;
}

static ERL_NIF_TERM mutate_batch_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return mutate_batch_impl(env, argv, 0);
}

/* mutate_batch_diffs(state, version, node, ops) -> {:ok, version', new_dots, changed, diffs}:
 * mutate_batch plus on_diffs' list for the batch's net changes (dgr_mutate_batch_diffs) */
static ERL_NIF_TERM mutate_batch_diffs_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  return mutate_batch_impl(env, argv, 1);
}

/* read(state, version, keys | :all) -> {:ok, %{key => value}}  (read/1,2, :211-224) */
static ERL_NIF_TERM read_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  if (!get_state(env, argv[0], argv[1], &s, &version)) return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  uint64_t *keys = NULL, n_keys = 0, n = 0;
  const uint64_t *hk = NULL, *hv = NULL;
  ERL_NIF_TERM r, m = enif_make_new_map(env);
  const int all = enif_is_identical(argv[2], A_ALL);
  if (!all) TRY(marshal_keys(env, g, argv[2], &keys, &n_keys));
  TRY(dgr_read(s->s, version, all, keys, n_keys, &hk, &hv, &n));
  for (uint64_t i = 0; i < n; i++) {
    const boxed* k = (const boxed*)dgm_key_term(g->u, hk[i]);
    ERL_NIF_TERM v;
    TRY(value_term(env, g, hv[i], &v));
    enif_make_map_put(env, m, enif_make_copy(env, k->t), v, &m);
  }
out:
  r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, m);
  if (keys) enif_free(keys);
  enif_mutex_unlock(g->lock);
  return r;
}

/* take(state, version, keys) -> {:ok, value map of those keys}  (Map.take, :118,331) */
static ERL_NIF_TERM take_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  if (!get_state(env, argv[0], argv[1], &s, &version)) return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  uint64_t *keys = NULL, n_keys = 0;
  dg_store taken;
  ERL_NIF_TERM r, values = A_NIL;
  TRY(marshal_keys(env, g, argv[2], &keys, &n_keys));
  TRY(dgr_take(s->s, version, keys, n_keys, &taken));
  TRY(unmarshal_host_rows(env, g, &taken, &values));
out:
  r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, values);
  if (keys) enif_free(keys);
  enif_mutex_unlock(g->lock);
  return r;
}

/* take_batch(state, version, [keys, ...]) -> {:ok, [value map, ...]}: take/3 for k pending
 * get_diff / send_diff messages, one dgr_take_batch per 64 keysets.  Every row of the keysets'
 * union comes home and becomes terms ONCE; the messages that hold a key share its value map. */
#define TAKE_BATCH_MAX 64
static ERL_NIF_TERM take_batch_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  unsigned total;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_list_length(env, argv[2], &total))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  uint64_t* keys[TAKE_BATCH_MAX];
  uint64_t n_keys[TAKE_BATCH_MAX];
  memset(keys, 0, sizeof keys);
  ERL_NIF_TERM* maps = (ERL_NIF_TERM*)enif_alloc((total ? total : 1) * sizeof *maps);
  ERL_NIF_TERM r, h, t = argv[2];
  unsigned done = 0;
  if (!maps) TRY(DG_E_NOMEM);
  while (done < total) {
    int k = 0;
    while (k < TAKE_BATCH_MAX && enif_get_list_cell(env, t, &h, &t)) {
      TRY(marshal_keys(env, g, h, &keys[k], &n_keys[k]));
      k++;
    }
    if (k == 0) TRY(DG_E_INVAL);
    dgr_taken tk;
    ERL_NIF_TERM values;
    TRY(dgr_take_batch(s->s, version, k, (const uint64_t* const*)keys, n_keys, &tk));
    TRY(unmarshal_host_rows(env, g, &tk.rows, &values));
    for (int j = 0; j < k; j++) maps[done + j] = enif_make_new_map(env);
    for (uint64_t i = 0; i < tk.n_keys; i++) {
      if (tk.offs[i + 1] == tk.offs[i]) continue; /* the state lacks the key */
      const ERL_NIF_TERM kt = key_term(env, g, tk.keys[i]);
      ERL_NIF_TERM ents;
      if (!enif_get_map_value(env, values, kt, &ents)) TRY(DG_E_INVAL);
      for (int j = 0; j < k; j++)
        if (tk.masks[i] >> j & 1) enif_make_map_put(env, maps[done + j], kt, ents, &maps[done + j]);
    }
    for (int j = 0; j < k; j++) {
      enif_free(keys[j]);
      keys[j] = NULL;
    }
    done += (unsigned)k;
  }
out:
  r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, enif_make_list_from_array(env, maps, total));
  for (int j = 0; j < TAKE_BATCH_MAX; j++)
    if (keys[j]) enif_free(keys[j]);
  if (maps) enif_free(maps);
  enif_mutex_unlock(g->lock);
  return r;
}

/* merkle_build(state, version, depth) -> :ok  (MerkleMap.new + put of every key, :21) */
static ERL_NIF_TERM merkle_build_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  unsigned depth;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_uint(env, argv[2], &depth))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = refresh_terms(g);
  if (!rc) rc = dgr_merkle_build(s->s, version, depth);
  ERL_NIF_TERM r = rc ? error_term(env, rc) : A_OK;
  enif_mutex_unlock(g->lock);
  return r;
}

/* sweep(engine) -> {:ok, %{values: {before, after}, keys: {before, after}}}: the value and
 * key terms no live state of the engine names any more are dropped from the universe
 * (dgr_sweep marks on the device, dgm_sweep_values / dgm_sweep_keys drop).  Under the engine
 * mutex: no delta is between its interning and its join.  State versions do not change. */
static ERL_NIF_TERM sweep_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  engine_res* g;
  if (!enif_get_resource(env, argv[0], ENGINE_RT, (void**)&g)) return enif_make_badarg(env);
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  const uint64_t *ids, *hash;
  const uint8_t* used;
  uint64_t n, n_used, unknown, dropped;
  const uint64_t v0 = dgm_value_count(g->u), k0 = dgm_key_count(g->u);
  dgm_value_hashes(g->u, &ids, &hash, &n);
  TRY(dgr_sweep(g->r, DG_COL_VAL, ids, n, &used, &n_used, &unknown));
  if (unknown) TRY(DG_E_INVAL); /* a state holds a value id the table lacks: drop nothing */
  TRY(dgm_sweep_values(g->u, used, n, &dropped));
  TRY(dgm_key_ids_sorted(g->u, &ids, &n));
  TRY(dgr_sweep(g->r, DG_COL_KEY, ids, n, &used, &n_used, &unknown));
  if (unknown) TRY(DG_E_INVAL);
  TRY(dgm_sweep_keys(g->u, ids, used, n, &dropped));
out:;
  ERL_NIF_TERM r;
  if (rc) {
    r = error_term(env, rc);
  } else {
    ERL_NIF_TERM m = enif_make_new_map(env);
    enif_make_map_put(env, m, enif_make_atom(env, "values"),
                      enif_make_tuple2(env, enif_make_uint64(env, v0),
                                       enif_make_uint64(env, dgm_value_count(g->u))), &m);
    enif_make_map_put(env, m, enif_make_atom(env, "keys"),
                      enif_make_tuple2(env, enif_make_uint64(env, k0),
                                       enif_make_uint64(env, dgm_key_count(g->u))), &m);
    r = enif_make_tuple2(env, A_OK, m);
  }
  enif_mutex_unlock(g->lock);
  return r;
}

static ERL_NIF_TERM bytes_term(ErlNifEnv* env, const uint8_t* p, uint64_t n) {
  ERL_NIF_TERM t;
  unsigned char* d = enif_make_new_binary(env, n, &t);
  memcpy(d, p, n);
  return t;
}

/* merkle_prepare(state, version, levels) -> {:continue, cont}  (:255) */
static ERL_NIF_TERM merkle_prepare_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  unsigned levels;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_uint(env, argv[2], &levels))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  const uint8_t* bin = NULL;
  uint64_t len = 0;
  const int rc = dgr_merkle_prepare(s->s, version, levels, &bin, &len);
  ERL_NIF_TERM r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_CONTINUE, bytes_term(env, bin, len));
  enif_mutex_unlock(g->lock);
  return r;
}

/* merkle_continue(state, version, cont, levels, max_sync_size | :infinite)
 *   -> {:continue, cont} | {:ok, keys}  (continue_partial_diff + truncate, :96-105,206-214) */
static ERL_NIF_TERM merkle_continue_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  ErlNifBinary in;
  unsigned levels;
  ErlNifUInt64 max_sync = UINT64_MAX;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_inspect_binary(env, argv[2], &in) ||
      !enif_get_uint(env, argv[3], &levels) ||
      (!enif_is_identical(argv[4], A_INFINITE) && !enif_get_uint64(env, argv[4], &max_sync)))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK, status = 0;
  const uint8_t* bin = NULL;
  const uint64_t* keys = NULL;
  uint64_t len = 0, n_keys = 0;
  ERL_NIF_TERM r = A_NIL;
  TRY(refresh_terms(g));
  TRY(dgr_merkle_continue(s->s, version, in.data, in.size, levels, max_sync, &status, &bin, &len, &keys,
                          &n_keys));
  if (status == 1) {
    r = enif_make_tuple2(env, A_CONTINUE, bytes_term(env, bin, len));
  } else {
    ERL_NIF_TERM l = enif_make_list(env, 0);
    for (uint64_t i = n_keys; i-- > 0;) l = enif_make_list_cell(env, key_term(env, g, keys[i]), l);
    r = enif_make_tuple2(env, A_OK, l);
  }
out:
  if (rc) r = error_term(env, rc);
  enif_mutex_unlock(g->lock);
  return r;
}

/* merkle_continue_batch(state, version, [cont, ...], levels, max_sync_size | :infinite)
 *   -> {:ok, [{:continue, cont} | {:ok, keys}, ...]}: merkle_continue/5 for k pending
 * {:diff, %Diff{continuation: ...}} messages, one dgr_merkle_continue_batch (one launch and one
 * wait for the messages within the one-workgroup limits) per 64.  Element j is what
 * merkle_continue/5 returns for message j, an {:error, _} included; all are answered against
 * the state as it is at the call, and a stale version fails the whole call. */
static ERL_NIF_TERM merkle_continue_batch_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  unsigned total, levels;
  ErlNifUInt64 max_sync = UINT64_MAX;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_list_length(env, argv[2], &total) ||
      !enif_get_uint(env, argv[3], &levels) ||
      (!enif_is_identical(argv[4], A_INFINITE) && !enif_get_uint64(env, argv[4], &max_sync)))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  const uint8_t* bins[DG_CONT_BATCH_MAX];
  uint64_t lens[DG_CONT_BATCH_MAX];
  dgr_cont_result res[DG_CONT_BATCH_MAX];
  ERL_NIF_TERM* out = (ERL_NIF_TERM*)enif_alloc((total ? total : 1) * sizeof *out);
  ERL_NIF_TERM r, h, t = argv[2];
  unsigned done = 0;
  if (!out) TRY(DG_E_NOMEM);
  TRY(refresh_terms(g));
  while (done < total) {
    int k = 0;
    while (k < DG_CONT_BATCH_MAX && enif_get_list_cell(env, t, &h, &t)) {
      ErlNifBinary in;
      if (!enif_inspect_binary(env, h, &in)) TRY(DG_E_INVAL);
      bins[k] = in.data;
      lens[k] = in.size;
      k++;
    }
    if (k == 0) TRY(DG_E_INVAL);
    TRY(dgr_merkle_continue_batch(s->s, version, k, bins, lens, levels, max_sync, res));
    for (int j = 0; j < k; j++) {
      if (res[j].rc) {
        out[done + j] = error_term(env, res[j].rc);
      } else if (res[j].status == 1) {
        out[done + j] = enif_make_tuple2(env, A_CONTINUE, bytes_term(env, res[j].bin, res[j].len));
      } else {
        ERL_NIF_TERM l = enif_make_list(env, 0);
        for (uint64_t i = res[j].n_keys; i-- > 0;) l = enif_make_list_cell(env, key_term(env, g, res[j].keys[i]), l);
        out[done + j] = enif_make_tuple2(env, A_OK, l);
      }
    }
    done += (unsigned)k;
  }
out:
  r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, enif_make_list_from_array(env, out, total));
  if (out) enif_free(out);
  enif_mutex_unlock(g->lock);
  return r;
}

/* merkle_continue_take_batch(state, version, [cont, ...], [want, ...], levels, max_sync_size | :infinite)
 *   -> {:ok, [{:continue, cont} | {:ok, keys} | {:ok, keys, value_map}, ...]}: merkle_continue_batch/5
 * that also answers send_diff (:324-335) for the messages whose `want` is true (the originator of
 * the sync: diff.originator != diff.to): where merkle_continue/5 gives {:ok, keys} with keys, the
 * element is {:ok, keys, value_map}, value_map what take/3 of those keys gives.  One
 * dgr_merkle_continue_take_batch per 64 messages: the rows come out of the hops' own launch. */
static ERL_NIF_TERM merkle_continue_take_batch_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  state_res* s;
  uint64_t version;
  unsigned total, n_want, levels;
  ErlNifUInt64 max_sync = UINT64_MAX;
  if (!get_state(env, argv[0], argv[1], &s, &version) || !enif_get_list_length(env, argv[2], &total) ||
      !enif_get_list_length(env, argv[3], &n_want) || n_want != total || !enif_get_uint(env, argv[4], &levels) ||
      (!enif_is_identical(argv[5], A_INFINITE) && !enif_get_uint64(env, argv[5], &max_sync)))
    return enif_make_badarg(env);
  engine_res* g = s->eng;
  enif_mutex_lock(g->lock);
  int rc = DG_OK;
  const uint8_t* bins[DG_CONT_BATCH_MAX];
  uint64_t lens[DG_CONT_BATCH_MAX];
  uint8_t want[DG_CONT_BATCH_MAX];
  dgr_cont_result res[DG_CONT_BATCH_MAX];
  dgr_hop_rows taken[DG_CONT_BATCH_MAX];
  const ERL_NIF_TERM a_true = enif_make_atom(env, "true");
  ERL_NIF_TERM* out = (ERL_NIF_TERM*)enif_alloc((total ? total : 1) * sizeof *out);
  ERL_NIF_TERM r, h, w, t = argv[2], tw = argv[3];
  unsigned done = 0;
  if (!out) TRY(DG_E_NOMEM);
  TRY(refresh_terms(g));
  while (done < total) {
    int k = 0;
    while (k < DG_CONT_BATCH_MAX && enif_get_list_cell(env, t, &h, &t) && enif_get_list_cell(env, tw, &w, &tw)) {
      ErlNifBinary in;
      if (!enif_inspect_binary(env, h, &in)) TRY(DG_E_INVAL);
      bins[k] = in.data;
      lens[k] = in.size;
      want[k] = enif_is_identical(w, a_true) ? 1 : 0;
      k++;
    }
    if (k == 0) TRY(DG_E_INVAL);
    TRY(dgr_merkle_continue_take_batch(s->s, version, k, bins, lens, want, levels, max_sync, res, taken));
    for (int j = 0; j < k; j++) {
      if (res[j].rc) {
        out[done + j] = error_term(env, res[j].rc);
      } else if (res[j].status == 1) {
        out[done + j] = enif_make_tuple2(env, A_CONTINUE, bytes_term(env, res[j].bin, res[j].len));
      } else {
        ERL_NIF_TERM l = enif_make_list(env, 0), values = A_NIL;
        for (uint64_t i = res[j].n_keys; i-- > 0;) l = enif_make_list_cell(env, key_term(env, g, res[j].keys[i]), l);
        if (want[j] && res[j].n_keys) {
          TRY(unmarshal_host_rows(env, g, &taken[j].rows, &values));
          out[done + j] = enif_make_tuple3(env, A_OK, l, values);
        } else {
          out[done + j] = enif_make_tuple2(env, A_OK, l);
        }
      }
    }
    done += (unsigned)k;
  }
out:
  r = rc ? error_term(env, rc) : enif_make_tuple2(env, A_OK, enif_make_list_from_array(env, out, total));
  if (out) enif_free(out);
  enif_mutex_unlock(g->lock);
  return r;
}

/* resolve_keys(engine, keys) -> keys: placeholders of keys this node knows -> their terms
 * (the others stay placeholders) */
static ERL_NIF_TERM resolve_keys_nif(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argc;
  engine_res* g;
  unsigned len;
  if (!enif_get_resource(env, argv[0], ENGINE_RT, (void**)&g) || !enif_get_list_length(env, argv[1], &len))
    return enif_make_badarg(env);
  enif_mutex_lock(g->lock);
  ERL_NIF_TERM* v = (ERL_NIF_TERM*)enif_alloc((len ? len : 1) * sizeof *v);
  ERL_NIF_TERM h, t = argv[1], r;
  unsigned n = 0;
  while (enif_get_list_cell(env, t, &h, &t)) {
    uint64_t id;
    v[n++] = placeholder_id(env, h, &id) ? key_term(env, g, id) : h;
  }
  r = enif_make_list_from_array(env, v, n);
  enif_free(v);
  enif_mutex_unlock(g->lock);
  return r;
}

/* ------------------------------------------------------------ load */
static int load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)priv;
  (void)info;
  ENGINE_RT = enif_open_resource_type(env, NULL, "deltagpu_engine", engine_dtor, ERL_NIF_RT_CREATE, NULL);
  STATE_RT = enif_open_resource_type(env, NULL, "deltagpu_state", state_dtor, ERL_NIF_RT_CREATE, NULL);
  A_OK = enif_make_atom(env, "ok");
  A_ERROR = enif_make_atom(env, "error");
  A_NIL = enif_make_atom(env, "nil");
  A_ALL = enif_make_atom(env, "all");
  A_CONTINUE = enif_make_atom(env, "continue");
  A_MAP = enif_make_atom(env, "map");
  A_STRUCT = enif_make_atom(env, "__struct__");
  A_MAPSET = enif_make_atom(env, "Elixir.MapSet");
  A_STALE = enif_make_atom(env, "stale");
  A_INFINITE = enif_make_atom(env, "infinite");
  A_DGKEY = enif_make_atom(env, "$dg_key");
  A_ADD = enif_make_atom(env, "add");
  A_REMOVE = enif_make_atom(env, "remove");
  return (ENGINE_RT && STATE_RT) ? 0 : 1;  /* a failed load -> the Elixir code path */
}

static ErlNifFunc funcs[] = {
    {"engine_open", 1, engine_open, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"state_load", 3, state_load, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"join_delta", 5, join_delta, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"mutate_batch", 4, mutate_batch_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"join_delta_diffs", 5, join_delta_diffs, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"sync_from", 5, sync_from_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"sync_from_diffs", 5, sync_from_diffs_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"mutate_batch_diffs", 4, mutate_batch_diffs_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"join_deltas", 3, join_deltas_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"join_deltas_diffs", 3, join_deltas_diffs_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"read", 3, read_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"take", 3, take_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"take_batch", 3, take_batch_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"merkle_build", 3, merkle_build_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"merkle_prepare", 3, merkle_prepare_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"merkle_continue", 5, merkle_continue_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"merkle_continue_batch", 5, merkle_continue_batch_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"merkle_continue_take_batch", 6, merkle_continue_take_batch_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"resolve_keys", 2, resolve_keys_nif, 0},
    {"sweep", 1, sweep_nif, ERL_NIF_DIRTY_JOB_CPU_BOUND},
};

ERL_NIF_INIT(Elixir.DeltaCrdt.GPU, funcs, load, NULL, NULL, NULL)
