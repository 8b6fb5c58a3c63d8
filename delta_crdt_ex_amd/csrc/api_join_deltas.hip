// api_join_deltas.hip — dg_store_diff and dg_join_deltas: the streaming diff of two stores
// (sdiff.hip), and a batch of k deltas joined into a resident state with everything
// CausalCrdt.update_state_with_delta needs from it -- the fold (api_fold.hip), the diff of
// the state before and after, the tree step, the context and the exchange of the stores.
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
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!state || !state_ctx || !spare || !n_changed || (cap && !changed) || k < 0 || (k > 0 && (!deltas || !dctxs)))
    return fail(DG_E_INVAL, "dg_join_deltas: bad argument");
  if (keys && !n_keys) return fail(DG_E_INVAL, "dg_join_deltas: keys without n_keys");
  *n_changed = 0;
  TRY(check_store(state, "dg_join_deltas state"));
  TRY(check_ctx(state_ctx, "dg_join_deltas state_ctx"));
  if (tree) TRY(check_merkle(tree, "dg_join_deltas tree"));
  TRY(check_diffs(diffs, cap, "dg_join_deltas"));
  TRY(check_rows_out(rows, "dg_join_deltas"));
  u64 total = state->n, total_ctx = state_ctx->n;
  for (int i = 0; i < k; i++) {
    TRY(check_store(&deltas[i], "dg_join_deltas delta"));
    TRY(check_ctx(&dctxs[i], "dg_join_deltas delta ctx"));
    if (keys && keys[i] == nullptr && n_keys[i] != 0) return fail(DG_E_INVAL, "dg_join_deltas: keys NULL with n_keys>0");
    total += deltas[i].n;
    total_ctx += dctxs[i].n;
  }
  if (k > 0 && spare->cap < total)
    return fail(DG_E_CAPACITY, "dg_join_deltas: spare cap %llu < %llu rows in", (unsigned long long)spare->cap,
                (unsigned long long)total);
  if (k > 0 && state_ctx->cap < total_ctx)
    return fail(DG_E_CAPACITY, "dg_join_deltas: state_ctx cap %llu < %llu", (unsigned long long)state_ctx->cap,
                (unsigned long long)total_ctx);
  if (k > 0 && total && (!spare->key || !spare->val || !spare->ts || !spare->node || !spare->cnt))
    return fail(DG_E_INVAL, "dg_join_deltas: null spare column");
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

}  // extern "C"
