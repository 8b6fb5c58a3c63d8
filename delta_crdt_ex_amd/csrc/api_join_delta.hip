// api_join_delta.hip — dg_join_delta and its forms: the one-wait path, the splice and full
// paths behind it, the home join, the diffs; and the tree update they share with
// dg_merkle_update.
#include "dg_engine.h"

namespace {

// MerkleMap put/delete + update_hashes of `keys` (the tree indexes `olds`; afterwards
// `news`), all or nothing: when the update meets an input error (a changed key outside the
// tree's shard, a bucket over 65535 rows) the same update with the stores exchanged
// restores every node and count bit for bit, and the error is returned.  `tail` enqueues
// work between the update and its host sync that must not take effect after a failed update
// (it reads the error word as a guard).  *d_n_keys = the change in distinct keys (not applied
// to t->n_keys).
template <class Tail>
int tree_update(dg_engine* e, dg_merkle* t, const dg_store* olds, const dg_store* news,
                const uint64_t* keys, uint64_t n_keys, const char* what, Tail tail, u64* d_n_keys) {
  TreeScratch ts;  // all of it in engine tmp; dirty and cdelta zeroed in one launch
  TRY(carve(e, &e->tmp, [&](Arena& m) { return tree_layout(m, m, merkle_ctr_words(t->depth), merkle_chunks(t->depth)); },
            &ts));
  u32* err = e->ticket + TK_INPUT;
  auto update = [&](const dg_store* from, const dg_store* to) -> int {
    HIP_TRY(launch_splice_finish(nullptr, nullptr, 0, nullptr, nullptr, ts.dirty, ts.zero_words, e->d_counts, err,
                                 e->stream));
    HIP_TRY(launch_merkle_update(merkle_of(t), rows_of(from), rows_of(to), keys, n_keys, ts.dirty, e->d_counts,
                                 e->ticket + MERKLE_ARRIVE, ts.hand, ts.cdelta, err, e->stream));
    return DG_OK;
  };
  TRY(update(olds, news));
  TRY(tail());
  TRY(read_counts(e));
  u64 dk = 0;
  for (int i = 0; i < TU_SHARDS; i++) dk += e->h_counts[i];  // signed changes, two's complement
  *d_n_keys = dk;
  const u32 bits = e->h_ticket[TK_INPUT];
  if (!(bits & MERKLE_INPUT_ERR)) return DG_OK;
  return undo_tree_update(e, tree_input_error(bits, what), err, [&] { return update(news, olds); });
}

}  // namespace

int tree_update(dg_engine* e, dg_merkle* t, const dg_store* olds, const dg_store* news,
                const uint64_t* keys, uint64_t n_keys, const char* what) {
  u64 dk = 0;
  TRY(tree_update(e, t, olds, news, keys, n_keys, what, [] { return (int)DG_OK; }, &dk));
  t->n_keys += dk;
  return DG_OK;
}

// ---- the one-wait chain's host half, shared by dg_join_delta (kd_count_kernel) and
//      dg_join_deltas_keyed (kk_count_kernel): everything of KdArgs but the delta side
//      (d, cd, cu_tmp), and what follows the count launch.
int kd_fill_args(dg_engine* e, KdArgs* pp, TreeScratch* ts, dg_store* state, dg_context* state_ctx,
                 const uint64_t* keys, u64 nk, const KdScratch& k, dg_store* spare, dg_merkle* tree, uint64_t* changed,
                 uint64_t cap, dg_store* rows, dg_context* ctx_out, const dg_lww_diffs* diffs) {
  KdArgs& p = *pp;
  p.a = rows_of(state);
  p.aw = rows_out_of(state);
  p.ca = ctx_of(state_ctx);
  p.ca_node = state_ctx->node;
  p.ca_cnt = state_ctx->cnt;
  p.ca_cap = state_ctx->cap;
  p.keys = keys;
  p.nk = nk;
  p.a_lo = k.a_lo;
  p.d_lo = k.d_lo;
  p.runs = k.runs;
  p.amask = k.amask;
  p.dmask = k.dmask;
  p.dh = k.dh;
  p.end = k.end;
  p.shift = k.shift;
  p.part = k.part;
  p.tile_u0 = k.tile_u0;
  p.uc_cnt = k.uctx.cnt;
  p.uc_node = k.uctx.node;
  if (diffs) {  // the per-key winners
    p.has_diffs = 1;
    p.dv_old = k.dv_old;
    p.dv_new = k.dv_new;
    p.old_val = diffs->old_val;
    p.new_val = diffs->new_val;
    p.dflags = diffs->flags;
  }
  p.ntiles = (nk + KD_BLOCK - 1) / KD_BLOCK;
  p.changed = changed;
  p.cap = cap;
  p.has_rows = rows != nullptr;
  if (rows) {
    p.rows = rows_out_of(rows);
    p.rows_cap = rows->cap;
  }
  p.sp = rows_out_of(spare);
  if (ctx_out) {
    p.co_node = ctx_out->node;
    p.co_cnt = ctx_out->cnt;
    p.co_cap = ctx_out->cap;
  }
  p.a_tiles = splice_tiles(state->n);
  p.has_tree = tree != nullptr;
  if (tree) p.t = merkle_of(tree);
  p.d_counts = e->d_counts;
  p.arrive = e->ticket + KD_ARRIVE;
  p.err = e->ticket + KD_ERR;
  // the tree update's scratch: hand-off words (engine scratch), and the dirty flags and
  // chunk row-count changes in a buffer of their own that stays zero between calls
  *ts = TreeScratch{};
  if (tree) {
    const u64 cw = merkle_ctr_words(tree->depth), chunks = merkle_chunks(tree->depth);
    Arena mh, mz;
    tree_layout(mh, mz, cw, chunks);
    TRY(ensure_tmp(e, mh.bytes()));
    TRY(ensure_kdz(e, mz.bytes()));
    Arena hand(e->tmp.p), flags(e->kdz.p);
    *ts = tree_layout(hand, flags, cw, chunks);
  }
  p.dirty = ts->dirty;
  p.cdelta = ts->cdelta;
  return DG_OK;
}

// Behind the count launch: the write beside the tree's re-reduction, the moved rows' copy, the
// ONE publish and wait, then the outcome.  *declined = the guard's KD_BAD | KD_BIG bits (the
// count kernel does not serve the input: nothing was written and the tree's put/delete has been
// undone; DG_OK); more changed keys than `cap` and a tree input error are returned, all or nothing.
int kd_finish_join(dg_engine* e, const KdArgs& p, const TreeScratch& ts, dg_store* state, dg_context* state_ctx,
                   dg_store* spare, dg_merkle* tree, uint64_t* n_changed, int* swapped, dg_store* rows,
                   dg_context* ctx_out, const char* what, u64* declined) {
  *declined = 0;
  u32* err = p.err;
  HIP_TRY(launch_kd_finish(p, ts.dirty, e->ticket + MERKLE_ARRIVE, ts.hand, ts.cdelta, e->stream));
  SpliceArgs sp{};
  sp.a = rows_of(state);
  sp.keys = p.keys;
  sp.nk = p.nk;
  sp.a_lo = p.a_lo;
  sp.end = p.end;
  sp.shift = p.shift;
  sp.tile_u0 = p.tile_u0;
  sp.out = rows_out_of(spare);
  sp.run_if = e->d_counts + KC_MOVED;
  sp.kguard = e->d_counts + KC_GUARD;
  sp.h_pub = e->d_pub;
  sp.pub_counts = e->d_counts;
  sp.seq = ++e->pub_seq;
  sp.arrive_all = e->ticket + SPL_ARRIVE;
  HIP_TRY(launch_splice_move(sp, e->stream));
  TRY(wait_published(e, sp.seq));
  TRY(published_errors(e));
  const u64 g = e->h_counts[KC_GUARD];
  const u32 tbits = e->h_ticket[KD_ERR];
  if (g || (tbits & MERKLE_INPUT_ERR)) {
    // nothing of the state or its context was written (the write kernel saw the guard or
    // the error word), but the count kernel put the changes into the tree: the same update
    // with the opposite sign restores every bucket node and count bit for bit.
    *declined = g & (KD_BAD | KD_BIG);
    const int rc = *declined ? DG_OK
                   : (g & KD_CAP) ? fail(DG_E_CAPACITY, "%s: %llu changed keys > cap %llu", what,
                                         (unsigned long long)e->h_counts[KC_CHANGED], (unsigned long long)p.cap)
                                  : tree_input_error(tbits, what);
    if (!tree) return rc;
    // (dirty and cdelta are zero again: the re-reduction consumed them)
    return undo_tree_update(e, rc, err, [&]() -> int {
      HIP_TRY(launch_kd_tree(merkle_of(tree), p.keys, p.runs, p.dh, p.nk, nullptr, -1, ts.dirty,
                             e->ticket + MERKLE_ARRIVE, ts.hand, ts.cdelta, err, e->stream));
      return DG_OK;
    });
  }
  if (e->h_counts[KC_MOVED]) {  // the state is in `spare`
    const u64 n = state->n - e->h_counts[KC_TAKEN] + e->h_counts[KC_EDIT];
    std::swap(*state, *spare);
    state->n = n;
    *swapped = 1;
  }
  state_ctx->n = e->h_counts[KC_CTX];
  state_ctx->kind = DG_CTX_VV;
  if (tree) tree->n_keys += e->h_counts[KC_DKEYS];
  *n_changed = e->h_counts[KC_CHANGED];
  if (rows) rows->n = e->h_counts[KC_ROWS];  // (more than rows->cap: not written, as the caller's contract says)
  if (ctx_out) {
    ctx_out->n = state_ctx->n;  // (more than ctx_out->cap: not written)
    ctx_out->kind = DG_CTX_VV;
  }
  return DG_OK;
}

extern "C" {

// dg_join_delta_rows' output: the changed keys' rows of `src`; more than rows->cap is
// reported in rows->n, not as an error (the join before it is complete).  It runs after
// the join is committed, so any failure of the gather is reported the same way -- "rows
// not written" (rows->n > rows->cap) -- and never as an error of a join that applied.
static int take_changed_rows(dg_engine* e, const dg_store* src, const uint64_t* changed,
                             uint64_t n_changed, dg_store* rows) {
  const int rc = dg_take_keys(e, src, changed, n_changed, rows);
  if (rc == DG_E_CAPACITY) return DG_OK;
  if (rc != DG_OK) rows->n = rows->cap + 1;
  return DG_OK;
}

// dg_join_delta_diffs' output on the paths that do not compute it in the join (the splice, the
// full join): dg_read_diff of the changed keys.  Like take_changed_rows it runs after the join
// is committed, so a failure is never the join's error: diffs->cap = 0 says "not written".
static int gather_diffs(dg_engine* e, const dg_store* olds, const dg_store* news, const uint64_t* changed,
                        uint64_t n_changed, dg_lww_diffs* diffs) {
  if (dg_read_diff(e, olds, news, changed, n_changed, diffs) != DG_OK) diffs->cap = 0;
  return DG_OK;
}

// dg_join_delta's one-wait path (kdelta.hip): count + scan, the context union, the tree's
// put/delete and re-reduction, the write (in place, or into `spare` with the moved rows'
// copy behind it), then ONE publish and wait.  *done = false and nothing changed when the
// delta has a row outside the keyset (the full join applies) or a key has more than KD_RUN
// rows on a side (the splice applies); a tree input error is undone before it returns.
static int kd_join_delta(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                         const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys, dg_store* spare,
                         dg_merkle* tree, uint64_t* changed, uint64_t cap, uint64_t* n_changed, int* swapped,
                         dg_store* rows, dg_context* ctx_out, const dg_lww_diffs* diffs, bool* done) {
  *done = false;
  if (!e->kd || n_keys == 0 || state_ctx->kind != DG_CTX_VV || state->cap < state->n ||
      !pair_aligned(state->key, state->val, state->ts, state->node, state->cnt) ||
      !pair_aligned(spare->key, spare->val, spare->ts, spare->node, spare->cnt))
    return DG_OK;
  const u64 nk = n_keys, ntiles = (nk + KD_BLOCK - 1) / KD_BLOCK, a_tiles = splice_tiles(state->n);
  const u64 uctx_cap = state_ctx->n + delta_ctx->n;
  KdScratch k;
  TRY(carve(e, &e->kdb, [&](Arena& m) {
    return kd_layout(m, nk, ntiles * KD_NV, a_tiles, uctx_cap, ctx_union_tmp_bytes(state_ctx->n, delta_ctx->n),
                     diffs != nullptr);
  }, &k));
  KdArgs p{};
  TreeScratch ts{};
  TRY(kd_fill_args(e, &p, &ts, state, state_ctx, keys, nk, k, spare, tree, changed, cap, rows, ctx_out, diffs));
  p.d = rows_of(delta);
  p.cd = ctx_of(delta_ctx);
  p.cu_tmp = k.cu_tmp;
  // three launches, one wait: the count (the per-key joins, the tree's put/delete, the scan
  // and the context union by its last workgroup), the write beside the tree's re-reduction,
  // the moved rows' copy (its last workgroup publishes the count block)
  HIP_TRY(launch_kd_join(p, e->stream));
  u64 declined = 0;
  TRY(kd_finish_join(e, p, ts, state, state_ctx, spare, tree, n_changed, swapped, rows, ctx_out, "dg_join_delta",
                     &declined));
  *done = declined == 0;
  return DG_OK;
}

// dg_join_delta[_rows]: rows (optional) receives the changed keys' joined rows
// ctx_out (optional): a copy of the joined context
static int join_delta_core(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                           const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                           dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                           uint64_t* n_changed, int* swapped, dg_store* rows, dg_context* ctx_out, bool* kd_done,
                           dg_lww_diffs* diffs = nullptr) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!swapped || !n_changed || (cap && !changed) || !spare || !state || !state_ctx)
    return fail(DG_E_INVAL, "dg_join_delta: null argument");
  *swapped = 0;
  *n_changed = 0;
  TRY(check_store(state, "dg_join_delta state"));
  TRY(check_store(delta, "dg_join_delta delta"));
  TRY(check_ctx(state_ctx, "dg_join_delta state_ctx"));
  TRY(check_ctx(delta_ctx, "dg_join_delta delta_ctx"));
  if (tree) TRY(check_merkle(tree, "dg_join_delta tree"));
  if (keys == nullptr && n_keys != 0) return fail(DG_E_INVAL, "dg_join_delta: keys NULL with n_keys>0");
  if (spare->cap < state->n + delta->n)
    return fail(DG_E_CAPACITY, "dg_join_delta: spare cap %llu < %llu rows in",
                (unsigned long long)spare->cap, (unsigned long long)(state->n + delta->n));
  if (state_ctx->cap < state_ctx->n + delta_ctx->n)
    return fail(DG_E_CAPACITY, "dg_join_delta: state_ctx cap %llu < %llu",
                (unsigned long long)state_ctx->cap, (unsigned long long)(state_ctx->n + delta_ctx->n));
  TRY(set_device(e));
  TRY(settle(e));
  // All or nothing: nothing of *state, *state_ctx or the tree changes unless the call
  // succeeds.  Everything that can fail (the join's grid, the capacity of `changed`, the
  // tree update's input checks) runs on scratch and `spare` first; the state is written
  // last, by kernels that skip their writes when the tree update reported an error.
  const u64 uctx_cap = state_ctx->n + delta_ctx->n;
  const dg_context_kind out_kind =
      (state_ctx->kind == DG_CTX_DOTS && delta_ctx->kind == DG_CTX_DOTS) ? DG_CTX_DOTS : DG_CTX_VV;
  {
    bool done = false;
    TRY(kd_join_delta(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed, cap,
                      n_changed, swapped, rows, ctx_out, diffs, &done));
    *kd_done = done;
    if (done) return DG_OK;
  }
  Splice w;
  bool ok = false;
  const dg_store old_state = *state;
  if (splice_wanted(e, state, delta, keys, n_keys, spare) && state->cap >= state->n)
    TRY(splice_take(e, state, delta, keys, n_keys, uctx_cap, &w, &ok));
  if (!ok) {
    // the full keyed join into the spare store (the merge, or a splice into `spare` that
    // dg_join2_changes picks itself), the context into its own scratch, then the tree
    dg_context uc;
    TRY(carve(e, &e->ubuf, [&](Arena& m) { return m.context(uctx_cap); }, &uc));
    TRY(dg_join2_changes(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, &uc,
                         changed, cap, n_changed));
    if (tree) TRY(tree_update(e, tree, &old_state, spare, changed, *n_changed, "dg_join_delta"));
    HIP_TRY(hipMemcpyAsync(state_ctx->node, uc.node, uc.n * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(state_ctx->cnt, uc.cnt, uc.n * 8, hipMemcpyDeviceToDevice, e->stream));
    TRY(read_counts(e));
    state_ctx->n = uc.n;
    state_ctx->kind = uc.kind;
    std::swap(*state, *spare);
    *swapped = 1;
    if (rows) TRY(take_changed_rows(e, state, changed, *n_changed, rows));  // (the new state)
    // (the old rows are still where they were: the join wrote the spare store)
    if (diffs) TRY(gather_diffs(e, &old_state, state, changed, *n_changed, diffs));
    return DG_OK;
  }
  TRY(splice_edit(e, &w, state_ctx, delta, delta_ctx, keys, n_keys, &w.uctx, true, changed, cap));
  if (const int rc0 = read_counts(e); rc0 != DG_OK) {
    // the join grid could not become resident (another process's persistent kernels) or
    // timed out: nothing of the state is written yet, so re-run the edit on a small grid,
    // as dg_join2_changes does.  Any other failure (a HIP error, a lost publish) is the
    // call's error, its message kept.
    if (!(e->last_err_bits & 3u)) return rc0;
    TRY(with_small_grid(e, [&]() -> int {
      HIP_TRY(hipMemsetAsync(e->d_counts + SC_MOVED, 0, sizeof(u64), e->stream));
      return splice_edit(e, &w, state_ctx, delta, delta_ctx, keys, n_keys, &w.uctx, true, changed, cap);
    }));
    TRY(read_counts(e));
  }
  const bool moved = (u32)e->h_counts[SC_MOVED] != 0;
  const u64 n_e = e->h_counts[JC_ROWS];
  w.uctx.n = e->h_counts[JC_CTX];
  *n_changed = e->h_counts[JC_CHANGED];
  if (*n_changed > cap)
    return fail(DG_E_CAPACITY, "dg_join_delta: %llu changed keys > cap %llu",
                (unsigned long long)*n_changed, (unsigned long long)cap);
  dg_store* out = moved ? spare : state;
  w.sp.out = rows_out_of(out);
  // the copy: into `spare` (scratch until the swap) when rows move, else E's rows in place,
  // guarded by the tree update's error word; then the union context, guarded the same way
  const u32* guard = tree ? e->ticket + TK_INPUT : nullptr;
  w.sp.guard = moved ? nullptr : guard;
  auto copy = [&]() -> int {
    HIP_TRY(launch_splice_copy(w.sp, !moved, e->stream));
    HIP_TRY(launch_splice_finish(w.uctx.node, w.uctx.cnt, w.uctx.n, state_ctx->node, state_ctx->cnt,
                                 nullptr, 0, nullptr, nullptr, e->stream, guard));
    return DG_OK;
  };
  dg_store ed = w.ed;  // the keyset's joined rows (scratch, key order)
  ed.n = n_e;
  if (tree) {
    // MerkleMap.put/delete of the changed keys: every changed key is a keyset key, so its
    // old rows are among the taken rows and its new rows among the edit's (both small and
    // cache-resident: no search of the 12.5M-row state)
    u64 dk = 0;
    TRY(tree_update(e, tree, &w.ak, &ed, changed, *n_changed, "dg_join_delta", copy, &dk));
    tree->n_keys += dk;
  } else {
    TRY(copy());
    TRY(read_counts(e));
  }
  out->n = old_state.n - w.n_ak + n_e;
  state_ctx->n = w.uctx.n;
  state_ctx->kind = out_kind;
  if (moved) {
    std::swap(*state, *spare);
    *swapped = 1;
  }
  // the changed keys' rows from the edit (a changed key is a keyset key: all of its
  // joined rows are in the edit), not by a search of the state
  if (rows) TRY(take_changed_rows(e, &ed, changed, *n_changed, rows));
  // ... and their reads before and after from the taken rows and the edit (the same reason;
  // in place the state's own old rows are overwritten by now)
  if (diffs) TRY(gather_diffs(e, &w.ak, &ed, changed, *n_changed, diffs));
  return DG_OK;
}

// dg_join_delta_home: the fused small-delta join (small.hip) with ONE host wait.  States
// of up to SMALL_COPY_TILES splice tiles get the moved-rows copy in the tail launch behind
// the join (small.hip small_tail_kernel: the copy, then the publish),
// guarded by its `moved` word; a larger state whose rows moved copies after the wait.
constexpr u64 SMALL_COPY_TILES = 64;
static_assert(DIFF_MISMATCH == DG_DIFF_MISMATCH, "deltagpu.h and the diff kernels agree");
static_assert(CS_IN == DG_CONT_HOME_ENTRIES && CS_B == DG_CONT_HOME_BUCKETS && CONT_HOME + CS_HDR <= 24,
              "deltagpu.h's limits; the header fits the publish block");
static_assert(SMALL_O_KEYS == DG_HOME_KEYS &&SMALL_O_ROWS == DG_HOME_ROWS && SMALL_EDIT == DG_HOME_STRIDE &&
                  SMALL_O_CTX == DG_HOME_CTX && SMALL_NODES == DG_HOME_NODES && SMALL_WORDS == DG_HOME_WORDS &&
                  SMALL_FALLBACK == DG_HOME_FALLBACK,
              "the result block is the header's home layout");
static_assert(SMALL_PUB_TOUCHED > 16 && SMALL_PUB_TOUCHED < CONT_HOME, "a free word of the publish block");
static_assert(SMALL_O_DOLD == DG_HOME_DIFF_OLD && SMALL_O_DNEW == DG_HOME_DIFF_NEW &&
                  SMALL_O_DFLAGS == DG_HOME_DIFF_FLAGS && SMALL_DIFFS_WORDS == DG_HOME_DIFFS_WORDS &&
                  KD_DIFF_OLD == DG_DIFF_OLD && KD_DIFF_NEW == DG_DIFF_NEW,
              "the diff ranges behind it are the header's");

// dg_mutate_home's ops (dg_mutate_batch's arrays): the delta and the keyset the kernel builds
struct MutOps {
  u32 node;
  u64 m;
  const uint8_t* kind;
  const u64 *key, *val;
  const i64* ts;
  const u64* rank;
  u64 n_adds;
};

// dg_join_delta_home (diffs false) and dg_join_delta_home_diffs: one body, two kernels; and
// with `mu` (delta, delta_ctx and keys null) dg_mutate_home[_diffs]: the same body on the
// kernels' mutation form, the keyset being at most mu->m keys the kernel leaves in scratch
static int join_delta_home_impl(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                                const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                                dg_store* spare, dg_merkle* tree, uint64_t* home, int* swapped, bool diffs,
                                const MutOps* mu = nullptr) {
  const char* const what = mu ? "dg_mutate_home" : "dg_join_delta_home";
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!swapped || !spare || !state || !state_ctx || !home) return fail(DG_E_INVAL, "%s: null argument", what);
  *swapped = 0;
  home[HW_FLAGS] = SMALL_FALLBACK;
  bool small;
  if (mu) {
    TRY(check_store(state, "dg_mutate_home state"));
    TRY(check_ctx(state_ctx, "dg_mutate_home state_ctx"));
    if (tree) TRY(check_merkle(tree, "dg_mutate_home tree"));
    if (mu->m && (!mu->kind || !mu->key || !mu->val || !mu->ts || !mu->rank))
      return fail(DG_E_INVAL, "dg_mutate_home: null argument");
    if (mu->n_adds > mu->m) return fail(DG_E_INVAL, "dg_mutate_home: n_adds > m");
    // (the touched keys are counted on the device: the kernel holds spare->cap against them)
    small = mu->m <= SMALL_KEYS && mu->node < SMALL_NODES && state_ctx->cap >= state_ctx->n + 1;
  } else {
    TRY(check_store(state, "dg_join_delta_home state"));
    TRY(check_store(delta, "dg_join_delta_home delta"));
    TRY(check_ctx(state_ctx, "dg_join_delta_home state_ctx"));
    TRY(check_ctx(delta_ctx, "dg_join_delta_home delta_ctx"));
    if (tree) TRY(check_merkle(tree, "dg_join_delta_home tree"));
    if (keys == nullptr && n_keys != 0) return fail(DG_E_INVAL, "dg_join_delta_home: keys NULL with n_keys>0");
    small = n_keys <= SMALL_KEYS && delta->n <= SMALL_DELTA && delta_ctx->n <= SMALL_DCTX &&
            spare->cap >= state->n + delta->n && state_ctx->cap >= 1;
  }
  small = small && state_ctx->kind == DG_CTX_VV && state_ctx->n <= SMALL_NODES && spare->cap >= state->n &&
          pair_aligned(state->key, state->val, state->ts, state->node, state->cnt) &&
          pair_aligned(spare->key, spare->val, spare->ts, spare->node, spare->cnt);
  if (!small) return DG_OK;  // home[0] = SMALL_FALLBACK: the caller takes dg_join_delta_rows
  TRY(set_device(e));
  TRY(settle(e));
  const u64 nk = mu ? mu->m : n_keys, a_tiles = splice_tiles(state->n);
  const bool copy_now = a_tiles <= SMALL_COPY_TILES;
  HomeScratch h;
  TRY(carve(e, &e->sml, [&](Arena& m) { return home_layout(m, SMALL_EDIT, nk, a_tiles, SMALL_WORDS); }, &h));
  dg_store ed = h.ed;
  u64 *a_lo = h.idx.a_lo, *a_off = h.idx.a_off, *end = h.idx.end, *tile_u0 = h.tile_u0, *res = h.res;
  i64 *shift = h.idx.shift, *gap = h.idx.gap;
  SmallArgs p{};
  p.a = rows_of(state);
  p.aw = rows_out_of(state);
  p.ca = ctx_of(state_ctx);
  p.ca_node = state_ctx->node;
  p.ca_cnt = state_ctx->cnt;
  p.ca_cap = state_ctx->cap;
  if (mu) {
    keys = h.keys;
    p.m_kind = mu->kind;
    p.m_key = mu->key;
    p.m_val = mu->val;
    p.m_ts = mu->ts;
    p.m_rank = mu->rank;
    p.m = mu->m;
    p.n_adds = mu->n_adds;
    p.node = mu->node;
    p.sp_cap = spare->cap;
    p.keys_out = h.keys;
  } else {
    p.d = rows_of(delta);
    p.cd = ctx_of(delta_ctx);
    p.keys = keys;
    p.nk = nk;
  }
  p.e = rows_out_of(&ed);
  p.a_lo = a_lo;
  p.a_off = a_off;
  p.res = res;
  p.has_tree = tree != nullptr;
  if (tree) p.t = merkle_of(tree);  // MerkleMap.put/delete + update_hashes: in the join
  p.splice_here = copy_now;
  p.sp = rows_out_of(spare);
  p.end = end;
  p.shift = shift;
  p.home = home;
  p.d_counts = e->d_counts;
  p.h_pub = e->d_pub;
  p.seq = ++e->pub_seq;
  HIP_TRY(mu ? launch_small_mutate(p, diffs, e->stream) : launch_small_delta(p, diffs, e->stream));
  if (copy_now) {  // the moved rows' copy into the spare (if they moved: else it returns)
    SmallTailArgs ta{};
    ta.a = rows_of(state);
    ta.out = rows_out_of(spare);
    ta.end = end;
    ta.a_lo = a_lo;
    ta.shift = shift;
    ta.nk = nk;
    ta.tiles = a_tiles;
    ta.res = res;
    ta.d_counts = e->d_counts;
    ta.h_pub = e->d_pub;
    ta.seq = p.seq;
    ta.arrive_all = e->ticket + TAIL_ARRIVE;
    HIP_TRY(launch_small_tail(ta, e->stream));
  }
  TRY(wait_published(e, p.seq));  // the one wait (the result block is in `home` by then)
  SpliceArgs sp{};
  sp.a = rows_of(state);
  sp.keys = keys;
  sp.nk = nk;
  sp.a_lo = a_lo;
  sp.a_off = a_off;
  sp.end = end;
  sp.shift = shift;
  sp.gap = gap;
  sp.tile_u0 = tile_u0;
  sp.moved = h.moved;
  sp.e = rows_of(&ed);
  sp.e.n = SMALL_EDIT;  // a bound: the kernels read the count
  sp.d_ne = res + HW_EDIT;
  sp.out = rows_out_of(spare);
  sp.run_if = res + HW_MOVED;  // (0 also when the join fell back or failed)
  const u64 flags = home[HW_FLAGS];
  if (flags & SMALL_ORDER) {  // (the mutation form) nothing written
    home[HW_FLAGS] = SMALL_FALLBACK;
    return fail(DG_E_ORDER, "%s: ops are not sorted by key", what);
  }
  if (flags & SMALL_FALLBACK) return DG_OK;  // nothing written: the general path
  if (flags & MERKLE_INPUT_ERR) return tree_input_error((u32)flags, what, "would hold");
  const u64 n_e = home[HW_EDIT], n_ak = home[HW_TAKEN];
  if (mu) sp.nk = e->h_pub[SMALL_PUB_TOUCHED];  // the touched keys, counted by the kernel
  if (home[HW_MOVED]) {  // rows moved: the state is in `spare` (copied behind the join, or now)
    if (!copy_now) {
      HIP_TRY(launch_splice_index(sp, e->stream));
      HIP_TRY(launch_splice_copy(sp, false, e->stream));
      TRY(read_counts(e));
    }
    const u64 n = state->n - n_ak + n_e;
    std::swap(*state, *spare);
    state->n = n;
    *swapped = 1;
  }
  state_ctx->n = home[HW_CTX];
  state_ctx->kind = DG_CTX_VV;
  if (tree) tree->n_keys += home[HW_DKEYS];
  return DG_OK;
}

int dg_join_delta_home(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                       const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                       dg_store* spare, dg_merkle* tree, uint64_t* home, int* swapped) {
  return join_delta_home_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, home, swapped,
                              false);
}

int dg_join_delta_home_diffs(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                             const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                             dg_store* spare, dg_merkle* tree, uint64_t* home, int* swapped) {
  return join_delta_home_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, home, swapped,
                              true);
}

int dg_mutate_home(dg_engine* e, dg_store* state, dg_context* state_ctx, uint32_t node, uint64_t m,
                   const uint8_t* kind, const uint64_t* key, const uint64_t* val, const int64_t* ts,
                   const uint64_t* add_rank, uint64_t n_adds, dg_store* spare, dg_merkle* tree, uint64_t* home,
                   int* swapped) {
  const MutOps mu{node, m, kind, key, val, ts, add_rank, n_adds};
  return join_delta_home_impl(e, state, state_ctx, nullptr, nullptr, nullptr, 0, spare, tree, home, swapped, false,
                              &mu);
}

int dg_mutate_home_diffs(dg_engine* e, dg_store* state, dg_context* state_ctx, uint32_t node, uint64_t m,
                         const uint8_t* kind, const uint64_t* key, const uint64_t* val, const int64_t* ts,
                         const uint64_t* add_rank, uint64_t n_adds, dg_store* spare, dg_merkle* tree,
                         uint64_t* home, int* swapped) {
  const MutOps mu{node, m, kind, key, val, ts, add_rank, n_adds};
  return join_delta_home_impl(e, state, state_ctx, nullptr, nullptr, nullptr, 0, spare, tree, home, swapped, true,
                              &mu);
}

static int join_delta_impl(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                           const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                           dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                           uint64_t* n_changed, int* swapped, dg_store* rows, dg_context* ctx_out = nullptr,
                           dg_lww_diffs* diffs = nullptr) {
  bool kd_done = false;
  TRY(join_delta_core(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed, cap, n_changed,
                      swapped, rows, ctx_out, &kd_done, diffs));
  if (ctx_out && !kd_done) {  // (the other paths: the context copied after the join)
    ctx_out->n = state_ctx->n;
    ctx_out->kind = state_ctx->kind;
    if (state_ctx->n <= ctx_out->cap && state_ctx->n) {
      HIP_TRY(hipMemcpyAsync(ctx_out->node, state_ctx->node, state_ctx->n * 4, hipMemcpyDefault, e->stream));
      HIP_TRY(hipMemcpyAsync(ctx_out->cnt, state_ctx->cnt, state_ctx->n * 8, hipMemcpyDefault, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
  }
  return DG_OK;
}

int dg_join_delta(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                  const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                  dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                  uint64_t* n_changed, int* swapped) {
  return join_delta_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed,
                         cap, n_changed, swapped, nullptr);
}

int dg_join_delta_rows(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                       const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                       dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                       uint64_t* n_changed, int* swapped, dg_store* rows) {
  if (!rows) return fail(DG_E_INVAL, "dg_join_delta_rows: null rows");
  return join_delta_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed,
                         cap, n_changed, swapped, rows);
}

int dg_join_delta_out(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                      const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                      dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                      uint64_t* n_changed, int* swapped, dg_store* rows, dg_context* ctx_out) {
  if (!rows || !ctx_out) return fail(DG_E_INVAL, "dg_join_delta_out: null rows or ctx_out");
  return join_delta_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed,
                         cap, n_changed, swapped, rows, ctx_out);
}

static_assert(KD_DIFF_OLD == DG_DIFF_OLD && KD_DIFF_NEW == DG_DIFF_NEW, "deltagpu.h's flags are the kernels'");

int dg_read_diff(dg_engine* e, const dg_store* old_s, const dg_store* new_s, const uint64_t* keys,
                 uint64_t n_keys, dg_lww_diffs* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(old_s, "dg_read_diff old"));
  TRY(check_store(new_s, "dg_read_diff new"));
  if (!out) return fail(DG_E_INVAL, "dg_read_diff: null output");
  if (keys == nullptr && n_keys != 0) return fail(DG_E_INVAL, "dg_read_diff: keys NULL with n_keys>0");
  if (out->cap < n_keys)
    return fail(DG_E_CAPACITY, "dg_read_diff: cap %llu < %llu keys", (unsigned long long)out->cap,
                (unsigned long long)n_keys);
  if (n_keys && (!out->old_val || !out->new_val || !out->flags)) return fail(DG_E_INVAL, "dg_read_diff: null output array");
  if (n_keys == 0) return DG_OK;
  TRY(set_device(e));
  TRY(settle(e));
  HIP_TRY(launch_read_diff(rows_of(old_s), rows_of(new_s), keys, n_keys, out->old_val, out->new_val, out->flags,
                           e->stream));
  return read_counts(e);
}

int dg_join_delta_diffs(dg_engine* e, dg_store* state, dg_context* state_ctx, const dg_store* delta,
                        const dg_context* delta_ctx, const uint64_t* keys, uint64_t n_keys,
                        dg_store* spare, dg_merkle* tree, uint64_t* changed, uint64_t cap,
                        uint64_t* n_changed, int* swapped, dg_store* rows, dg_context* ctx_out,
                        dg_lww_diffs* diffs) {
  if (!diffs) return fail(DG_E_INVAL, "dg_join_delta_diffs: null diffs");
  if (diffs->cap < cap)
    return fail(DG_E_INVAL, "dg_join_delta_diffs: diffs cap %llu < changed cap %llu",
                (unsigned long long)diffs->cap, (unsigned long long)cap);
  if (cap && (!diffs->old_val || !diffs->new_val || !diffs->flags))
    return fail(DG_E_INVAL, "dg_join_delta_diffs: null diffs array");
  return join_delta_impl(e, state, state_ctx, delta, delta_ctx, keys, n_keys, spare, tree, changed,
                         cap, n_changed, swapped, rows, ctx_out, diffs);
}

}  // extern "C"
