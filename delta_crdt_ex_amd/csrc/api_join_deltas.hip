// api_join_deltas.hip — dg_store_diff and dg_join_deltas: the streaming diff of two stores
// (sdiff.hip), and a batch of k deltas joined into a resident state with everything
// CausalCrdt.update_state_with_delta needs from it -- the fold (api_fold.hip), the diff of
// the state before and after, the tree step, the context and the exchange of the stores.
// dg_join_deltas_keyed is the same batch at the cost of the keys it names, for small keyed
// deltas: the keysets' union, then dg_join_delta's one-wait path over it (kdelta.hip, kkeyed.hip).
//
// The changed keys are the batch's NET change: every key whose row set differs between the
// state before and after.  For sync- and mutation-shaped deltas (every delta row's key is in
// its keyset: the only shapes CausalCrdt makes) that is the union of the reference's per-delta
// diff/3 results, minus the keys that changed and changed back.  For any other shape it is a
// superset that also holds the keys carried over from outside the keysets, so the tree
// always equals a rebuild.  The diffs (on_diffs) are net over the batch in the same way.
#include "dg_engine.h"

namespace {

int check_diffs(const dg_lww_diffs* diffs, uint64_t cap, const char* what) {
  if (!diffs) return DG_OK;
  if (diffs->cap < cap)
    return fail(DG_E_INVAL, "%s: diffs cap %llu < changed cap %llu", what, (unsigned long long)diffs->cap,
                (unsigned long long)cap);
  if (cap && (!diffs->old_val || !diffs->new_val || !diffs->flags)) return fail(DG_E_INVAL, "%s: null diffs array", what);
  return DG_OK;
}

int check_rows_out(const dg_store* rows, const char* what) {
  if (rows && rows->cap && (!rows->key || !rows->val || !rows->ts || !rows->node || !rows->cnt))
    return fail(DG_E_INVAL, "%s: null rows column", what);
  return DG_OK;
}

// The argument checks dg_join_deltas and dg_join_deltas_keyed share; *total = the rows in
// (state and deltas), *total_ctx = the context entries in.
int check_batch(const char* what, dg_engine* e, const dg_store* state, const dg_context* state_ctx, int k,
                const dg_store* deltas, const dg_context* dctxs, const uint64_t* const* keys, const uint64_t* n_keys,
                const dg_store* spare, const dg_merkle* tree, const uint64_t* changed, uint64_t cap,
                uint64_t* n_changed, const dg_store* rows, const dg_lww_diffs* diffs, u64* total_out,
                u64* total_ctx_out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!state || !state_ctx || !spare || !n_changed || (cap && !changed) || k < 0 || (k > 0 && (!deltas || !dctxs)))
    return fail(DG_E_INVAL, "%s: bad argument", what);
  if (keys && !n_keys) return fail(DG_E_INVAL, "%s: keys without n_keys", what);
  *n_changed = 0;
  const std::string w = what;
  TRY(check_store(state, (w + " state").c_str()));
  TRY(check_ctx(state_ctx, (w + " state_ctx").c_str()));
  if (tree) TRY(check_merkle(tree, (w + " tree").c_str()));
  TRY(check_diffs(diffs, cap, what));
  TRY(check_rows_out(rows, what));
  u64 total = state->n, total_ctx = state_ctx->n;
  for (int i = 0; i < k; i++) {
    TRY(check_store(&deltas[i], (w + " delta").c_str()));
    TRY(check_ctx(&dctxs[i], (w + " delta ctx").c_str()));
    if (keys && keys[i] == nullptr && n_keys[i] != 0) return fail(DG_E_INVAL, "%s: keys NULL with n_keys>0", what);
    total += deltas[i].n;
    total_ctx += dctxs[i].n;
  }
  if (k > 0 && spare->cap < total)
    return fail(DG_E_CAPACITY, "%s: spare cap %llu < %llu rows in", what, (unsigned long long)spare->cap,
                (unsigned long long)total);
  if (k > 0 && state_ctx->cap < total_ctx)
    return fail(DG_E_CAPACITY, "%s: state_ctx cap %llu < %llu", what, (unsigned long long)state_ctx->cap,
                (unsigned long long)total_ctx);
  if (k > 0 && total && (!spare->key || !spare->val || !spare->ts || !spare->node || !spare->cnt))
    return fail(DG_E_INVAL, "%s: null spare column", what);
  *total_out = total;
  *total_ctx_out = total_ctx;
  return DG_OK;
}

// The diff enqueued and waited for: *nk changed keys (the first min(*nk, cap) written, with
// their diffs), *nr their rows in new_s (written when they fit rows->cap).  Only reads the
// stores; its scratch is engine tmp.
int store_diff_core(dg_engine* e, const dg_store* old_s, const dg_store* new_s, uint64_t* changed, uint64_t cap,
                    dg_store* rows, const dg_lww_diffs* diffs, u64* nk, u64* nr) {
  const u64 tiles = sdiff_tiles(old_s->n, new_s->n), words = sdiff_mask_words(old_s->n, new_s->n);
  if (tiles >= (1ull << 31)) return fail(DG_E_INVAL, "dg_store_diff: %llu tiles", (unsigned long long)tiles);
  SdiffScratch s;
  TRY(carve(e, &e->tmp, [&](Arena& m) { return sdiff_layout(m, tiles, words); }, &s));
  SdiffArgs p{};
  p.a = rows_of(old_s);
  p.b = rows_of(new_s);
  p.ntiles = tiles;
  p.bounds = s.bounds;
  p.cnt_k = s.cnt_k;
  p.cnt_r = s.cnt_r;
  p.off_k = s.off_k;
  p.off_r = s.off_r;
  p.mask = s.mask;
  p.mask_words = words;
  p.changed = changed;
  p.cap = cap;
  if (rows) {
    p.has_rows = 1;
    p.rows = rows_out_of(rows);
    p.rows_cap = rows->cap;
  }
  if (diffs) {
    p.has_diffs = 1;
    p.old_val = diffs->old_val;
    p.new_val = diffs->new_val;
    p.flags = diffs->flags;
  }
  p.d_counts = e->d_counts;
  HIP_TRY(launch_store_diff(p, e->stream));
  TRY(read_counts(e));
  *nk = e->h_counts[SD_KEYS];
  *nr = e->h_counts[SD_ROWS];
  return DG_OK;
}

// The tree after a batch that changed a large share of the keys: dg_merkle_build's kernels on
// the new state (a stream, where the update re-hashes with a searched thread per key).  All
// or nothing: a build that meets an input error is followed by a build from the old store,
// which restores every node, count and chunk start bit for bit (the tree indexed that store).
int tree_rebuild(dg_engine* e, dg_merkle* t, const dg_store* olds, const dg_store* news) {
  auto build = [&](const dg_store* s) -> int {
    TRY(merkle_build_enqueue(e, s, t, e->d_counts));
    return read_counts(e);
  };
  TRY(build(news));
  const u32 bits = e->h_ticket[TK_INPUT];
  if (!(bits & MERKLE_INPUT_ERR)) {
    t->n_keys = e->h_counts[JC_ROWS];
    return DG_OK;
  }
  const int rc = tree_input_error(bits, "dg_join_deltas");
  const std::string msg = g_err;
  TRY(build(olds));
  g_err = msg;
  return rc;
}

}  // namespace

extern "C" {

int dg_store_diff(dg_engine* e, const dg_store* old_s, const dg_store* new_s, uint64_t* changed, uint64_t cap,
                  uint64_t* n_changed, dg_store* rows, dg_lww_diffs* diffs) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!n_changed || (cap && !changed)) return fail(DG_E_INVAL, "dg_store_diff: null argument");
  *n_changed = 0;
  TRY(check_store(old_s, "dg_store_diff old"));
  TRY(check_store(new_s, "dg_store_diff new"));
  TRY(check_diffs(diffs, cap, "dg_store_diff"));
  TRY(check_rows_out(rows, "dg_store_diff"));
  TRY(set_device(e));
  TRY(settle(e));
  u64 nk = 0, nr = 0;
  TRY(store_diff_core(e, old_s, new_s, changed, cap, rows, diffs, &nk, &nr));
  *n_changed = nk;
  if (rows) rows->n = nr;  // (more than rows->cap: not written)
  if (nk > cap)
    return fail(DG_E_CAPACITY, "dg_store_diff: %llu changed keys > cap %llu", (unsigned long long)nk,
                (unsigned long long)cap);
  return DG_OK;
}

int dg_join_deltas(dg_engine* e, dg_store* state, dg_context* state_ctx, int k, const dg_store* deltas,
                   const dg_context* dctxs, const uint64_t* const* keys, const uint64_t* n_keys, dg_store* spare,
                   dg_merkle* tree, uint64_t* changed, uint64_t cap, uint64_t* n_changed, dg_store* rows,
                   dg_context* ctx_out, dg_lww_diffs* diffs) {
  u64 total = 0, total_ctx = 0;
  TRY(check_batch("dg_join_deltas", e, state, state_ctx, k, deltas, dctxs, keys, n_keys, spare, tree, changed, cap,
                  n_changed, rows, diffs, &total, &total_ctx));
  TRY(set_device(e));
  TRY(settle(e));
  auto copy_ctx_out = [&](const dg_context* c) -> int {  // (more than ctx_out->cap: not written)
    if (!ctx_out) return DG_OK;
    ctx_out->n = c->n;
    ctx_out->kind = c->kind;
    if (c->n && c->n <= ctx_out->cap) {
      HIP_TRY(hipMemcpyAsync(ctx_out->node, c->node, c->n * 4, hipMemcpyDefault, e->stream));
      HIP_TRY(hipMemcpyAsync(ctx_out->cnt, c->cnt, c->n * 8, hipMemcpyDefault, e->stream));
    }
    return DG_OK;
  };
  if (k == 0) {  // nothing changes
    if (rows) rows->n = 0;
    TRY(copy_ctx_out(state_ctx));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return DG_OK;
  }
  // All or nothing.  The fold writes `spare` and engine scratch (the union context: ubuf), the
  // diff only reads, the tree step undoes itself; the state's context and the two store
  // structs are written last.
  dg_context uc;
  TRY(carve(e, &e->ubuf, [&](Arena& m) { return m.context(total_ctx); }, &uc));
  dg_store out = *spare;
  out.n = 0;
  TRY(apply_deltas(e, state, state_ctx, k, deltas, dctxs, keys, n_keys, &out, &uc));
  u64 nk = 0, nr = 0;
  TRY(store_diff_core(e, state, &out, changed, cap, rows, diffs, &nk, &nr));
  if (nk > cap)
    return fail(DG_E_CAPACITY, "dg_join_deltas: %llu changed keys > cap %llu", (unsigned long long)nk,
                (unsigned long long)cap);
  if (tree) {
    const bool rebuild = e->tree_rebuild == dg_engine::TREE_ALWAYS ||
                         (e->tree_rebuild == dg_engine::TREE_BY_SHARE && nk > out.n / e->tree_rebuild_div);
    if (rebuild)
      TRY(tree_rebuild(e, tree, state, &out));
    else
      TRY(tree_update(e, tree, state, &out, changed, nk, "dg_join_deltas"));
  }
  if (uc.n) {
    HIP_TRY(hipMemcpyAsync(state_ctx->node, uc.node, uc.n * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(state_ctx->cnt, uc.cnt, uc.n * 8, hipMemcpyDeviceToDevice, e->stream));
  }
  TRY(copy_ctx_out(&uc));
  HIP_TRY(hipStreamSynchronize(e->stream));
  state_ctx->n = uc.n;
  state_ctx->kind = uc.kind;
  const dg_store old = *state;
  *state = out;
  *spare = old;
  *n_changed = nk;
  if (rows) rows->n = nr;  // (more than rows->cap: not written)
  return DG_OK;
}

// The same batch at the cost of the keys it names (kkeyed.hip kk_count_kernel): the keysets'
// union with its masks as dg_take_keysets builds it (two waits: the keysets' order, the union's
// size), then dg_join_delta's one-wait path with the fold's count kernel in the place of the
// join's -- the VV tables, the count (each union key's candidates folded, its new rows into
// the edit store, the tree's put/delete), the write beside the tree's re-reduction, the moved
// rows' copy, ONE publish and wait.
int dg_join_deltas_keyed(dg_engine* e, dg_store* state, dg_context* state_ctx, int k, const dg_store* deltas,
                         const dg_context* dctxs, const uint64_t* const* keys, const uint64_t* n_keys,
                         dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap, uint64_t* n_changed,
                         dg_store* rows, dg_context* ctx_out, dg_lww_diffs* diffs, int* swapped) {
  if (!swapped) return fail(DG_E_INVAL, "dg_join_deltas_keyed: null swapped");
  *swapped = 0;
  u64 total = 0, total_ctx = 0;
  TRY(check_batch("dg_join_deltas_keyed", e, state, state_ctx, k, deltas, dctxs, keys, n_keys, spare, tree, changed,
                  cap, n_changed, rows, diffs, &total, &total_ctx));
  if (k == 0)  // nothing changes: dg_join_deltas' answer
    return dg_join_deltas(e, state, state_ctx, 0, deltas, dctxs, keys, n_keys, spare, tree, changed, cap, n_changed,
                          rows, ctx_out, diffs);
  // what the host can tell of a batch this path does not serve (the device finds the rest: a
  // delta row outside its keyset, a node id >= KNT, more than KD_RUN rows of a key)
  bool served = k <= KFOLD_MAX_K && keys && state_ctx->kind == DG_CTX_VV && state->cap >= state->n &&
                pair_aligned(state->key, state->val, state->ts, state->node, state->cnt) &&
                pair_aligned(spare->key, spare->val, spare->ts, spare->node, spare->cnt);
  u64 m = 0;
  for (int i = 0; served && i < k; i++) {
    served = keys[i] && dctxs[i].kind == DG_CTX_VV && deltas[i].n < (1ull << 32) && n_keys[i] < (1ull << 32);
    m += n_keys[i];
  }
  if (!served || m == 0 || m >= (1ull << 32)) return DG_KEYED_FALLBACK;
  TRY(set_device(e));
  TRY(settle(e));
  const u64 e_rows = total - state->n, a_tiles = splice_tiles(state->n);
  constexpr size_t HIST8_BYTES = 8 * 256 * sizeof(u32);  // sort_fields' pinned byte counts
  const size_t seg_bytes = (size_t)(k + 1) * sizeof(KsSeg), run_bytes = (size_t)k * sizeof(KRun);
  TRY(ensure_stage(e, HIST8_BYTES + seg_bytes + run_bytes));
  TRY(ensure_state(e, ks_tiles(m) + 1));
  KeyedScratch s;
  TRY(carve(e, &e->kdb, [&](Arena& a) {
    return keyed_layout(a, (u64)k, sizeof(KsSeg), sizeof(KRun), m, sort_tmp_bytes(m), KNT, e_rows,
                        (m + KD_BLOCK - 1) / KD_BLOCK * KD_NV, a_tiles, total_ctx, diffs != nullptr);
  }, &s));
  // ---- the union of the keysets, ascending, with per key the deltas that name it
  u32* h_hist8 = e->h_stage.as<u32>();
  KsSeg* hs = (KsSeg*)(e->h_stage.as<char>() + HIST8_BYTES);
  KRun* hr = (KRun*)(e->h_stage.as<char>() + HIST8_BYTES + seg_bytes);
  u64 off = 0;
  for (int i = 0; i < k; i++) {
    hs[i] = KsSeg{keys[i], off};
    off += n_keys[i];
    hr[i] = KRun{rows_of(&deltas[i]), keys[i], n_keys[i], ctx_of(&dctxs[i])};
  }
  hs[k] = KsSeg{nullptr, m};
  HIP_TRY(hipMemcpyAsync(s.segs, hs, seg_bytes, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(s.runs, hr, run_bytes, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemsetAsync(s.tabC, 0, s.zero_bytes, e->stream));
  u32* bad = e->ticket + TK_INPUT;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(u32), e->stream));
  // the items in (key, keyset) order: a few thousand by their ranks in the keysets (one launch,
  // no wait), more through the radix sort, whose order flag is waited for before it
  const bool by_rank = m * (u64)k <= KS_RANK_MAX;
  const char* unordered = "dg_join_deltas_keyed: a keyset is not strictly ascending";
  u32* idx = nullptr;
  if (by_rank) {
    HIP_TRY(launch_keysets_rank((const KsSeg*)s.segs, k, m, s.cat, s.set, bad, e->stream));
  } else {
    HIP_TRY(launch_keysets_gather((const KsSeg*)s.segs, k, m, s.cat, s.set, bad, e->stream));
    TRY(read_counts(e));
    if (e->h_ticket[TK_INPUT]) return fail(DG_E_ORDER, "%s", unordered);
    const SortField f{s.cat, 8, 0};
    HIP_TRY(sort_fields(&f, 1, m, s.sort_tmp, &idx, h_hist8, e->stream));
  }
  Scan sc;
  TRY(next_scan(e, &sc));
  constexpr int UNION_KEYS = 1;  // e->d_counts: the union's size (the join's count block comes after)
  HIP_TRY(launch_keysets_union(s.cat, s.set, idx, m, s.usorted, s.ukeys, s.masks, m, sc, e->d_counts + UNION_KEYS,
                               e->stream));
  TRY(read_counts(e));
  if (e->h_ticket[TK_INPUT]) return fail(DG_E_ORDER, "%s", unordered);  // (by_rank: found in the same wait)
  const u64 nk = e->h_counts[UNION_KEYS];
  if (nk == 0 || nk > m) return fail(DG_E_DEVICE, "dg_join_deltas_keyed: a union of %llu keys", (unsigned long long)nk);
  // ---- the join: dg_join_delta's one-wait chain over the union, d = the edit store
  KkArgs q{};
  TreeScratch ts{};
  TRY(kd_fill_args(e, &q.kd, &ts, state, state_ctx, s.ukeys, nk, s.kd, spare, tree, changed, cap, rows, ctx_out, diffs));
  dg_store ed = s.ed;
  ed.n = e_rows;
  q.kd.d = rows_of(&ed);
  q.masks = s.masks;
  q.runs = (const KRun*)s.runs;
  q.k = k;
  q.c0 = ctx_of(state_ctx);
  q.tabC = s.tabC;
  q.tabP = s.tabP;
  q.e = rows_out_of(&ed);
  q.e_rows = e_rows;
  q.e_next = s.e_next;
  q.flag = s.flag;
  HIP_TRY(launch_kk_join(q, e->stream));
  u64 declined = 0;
  TRY(kd_finish_join(e, q.kd, ts, state, state_ctx, spare, tree, n_changed, swapped, rows, ctx_out,
                     "dg_join_deltas_keyed", &declined));
  return declined ? (int)DG_KEYED_FALLBACK : (int)DG_OK;
}

}  // extern "C"
