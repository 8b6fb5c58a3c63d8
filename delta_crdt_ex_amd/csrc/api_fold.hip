// api_fold.hip — dg_joink and dg_apply_deltas: the delta-by-delta fold and the one-pass
// fold (kfold.hip).
#include "dg_engine.h"

namespace {

// Two intermediate states (rows + context) for a fold over at most `rows` rows and
// `ctx` context entries, carved from engine scratch that persists across calls.
int fold_buffers(dg_engine* e, u64 rows, u64 ctx, dg_store* st, dg_context* cx) {
  FoldScratch f;
  TRY(carve(e, &e->fold, [&](Arena& m) { return fold_layout(m, rows, ctx); }, &f));
  for (int w = 0; w < 2; w++) {
    st[w] = f.st[w];
    cx[w] = f.cx[w];
  }
  return DG_OK;
}

int copy_state(dg_engine* e, const dg_store* s, const dg_context* c, dg_store* out,
               dg_context* out_ctx) {
  if (out->cap < s->n || out_ctx->cap < c->n) return fail(DG_E_CAPACITY, "output capacity too small");
  if (s->n) TRY(copy_rows(e, out, s, s->n, hipMemcpyDeviceToDevice));
  if (c->n) {
    HIP_TRY(hipMemcpyAsync(out_ctx->node, c->node, c->n * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(out_ctx->cnt, c->cnt, c->n * 8, hipMemcpyDeviceToDevice, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  out->n = s->n;
  out_ctx->n = c->n;
  out_ctx->kind = c->kind;
  return DG_OK;
}

// acc <- join(acc, s_i, keys_i) for i = 0..k-1 (acc starts as (state, ctx)); the last
// step writes into out.
int fold_join(dg_engine* e, const dg_store* state, const dg_context* ctx, int k,
              const dg_store* stores, const dg_context* ctxs, const uint64_t* const* keys,
              const uint64_t* n_keys, dg_store* out, dg_context* out_ctx, const char* what) {
  u64 total = state->n, total_ctx = ctx->n;
  for (int s = 0; s < k; s++) {
    TRY(check_store(&stores[s], what));
    TRY(check_ctx(&ctxs[s], what));
    total += stores[s].n;
    total_ctx += ctxs[s].n;
  }
  if (out->cap < total || out_ctx->cap < total_ctx)
    return fail(DG_E_CAPACITY, "%s: output capacity too small (%llu rows, %llu ctx needed)", what,
                (unsigned long long)total, (unsigned long long)total_ctx);
  TRY(set_device(e));
  if (k == 0) return copy_state(e, state, ctx, out, out_ctx);
  dg_store buf[2];
  dg_context bufc[2];
  if (k > 1) TRY(fold_buffers(e, total, total_ctx, buf, bufc));
  dg_store acc = *state;
  dg_context acc_ctx = *ctx;
  for (int s = 0; s < k; s++) {
    dg_store* dst = (s == k - 1) ? out : &buf[s & 1];
    dg_context* dstc = (s == k - 1) ? out_ctx : &bufc[s & 1];
    dst->n = 0;
    const uint64_t* ks = keys ? keys[s] : nullptr;
    const uint64_t nk = (keys && keys[s]) ? n_keys[s] : 0;
    TRY(dg_join2(e, &acc, &acc_ctx, &stores[s], &ctxs[s], ks, nk, dst, dstc));
    acc = *dst;
    acc_ctx = *dstc;
  }
  return DG_OK;
}

// One pass of dg_apply_deltas over k <= KFOLD_MAX_K deltas (kfold.hip).  *stepwise is
// set when this input needs the delta-by-delta fold instead: a context that is not a
// version vector, a node id >= KNT, or a key bucket over its LDS capacity (keys far
// from uniform hashes).  The state and deltas are only read.
int kfold_pass(dg_engine* e, const dg_store* state, const dg_context* ctx, int k,
               const dg_store* deltas, const dg_context* dctxs, const uint64_t* const* keys,
               const uint64_t* n_keys, dg_store* out, dg_context* out_ctx, bool* stepwise) {
  *stepwise = true;
  if (k < 1 || k > KFOLD_MAX_K || ctx->kind != DG_CTX_VV) return DG_OK;
  u64 m_rows = 0, m_keys = 0, allmask = 0, dotsmask = 0, n_dots = 0;
  for (int i = 0; i < k; i++) {
    if (deltas[i].n >= (1ull << 32)) return DG_OK;
    if (dctxs[i].kind == DG_CTX_DOTS) {  // a mutation delta's MapSet context
      dotsmask |= 1ull << i;
      n_dots += dctxs[i].n;
    }
    const bool full = !keys || !keys[i];
    const u64 nk = full ? 0 : n_keys[i];
    if (nk >= (1ull << 32)) return DG_OK;
    if (full) allmask |= 1ull << i;
    m_rows += deltas[i].n;
    m_keys += nk;
  }
  auto ceil_div = [](u64 a, u64 b) { return (a + b - 1) / b; };
  const u64 T0 = std::max<u64>({ceil_div(state->n, KFOLD_MEAN_S), ceil_div(m_rows, KFOLD_MEAN_D),
                                ceil_div(m_keys, KFOLD_MEAN_M),
                                ceil_div(m_rows + m_keys, KFOLD_MEAN_U), 1});
  // a bucket over capacity (key groups far larger than the mean, or keys that are not
  // uniform hashes) is retried once with 8x the buckets
  for (int attempt = 0; attempt < 2; attempt++) {
    const u64 T = T0 << (3 * attempt);
    if (T >= (1ull << 31)) return DG_OK;
    u64 dset_n = 1024;  // a power of two at least twice the dots: probes stay short
    while (dset_n < 2 * n_dots) dset_n <<= 1;
    TRY(ensure_state(e, T + 2));
    KfoldScratch d;  // device scratch, its head staged in pinned memory
    TRY(carve(e, &e->tmp, [&](Arena& m) { return kfold_layout(m, k, sizeof(KRun), T, KNT, dotsmask ? dset_n : 0); },
              &d));
    TRY(ensure_stage(e, d.staged_bytes));
    Arena stage(e->h_stage.p);
    const KfoldStaged h = kfold_staged_layout(stage, k, sizeof(KRun));
    KRun* hr = (KRun*)h.runs;
    for (int i = 0; i < k; i++) {
      hr[i].rows = rows_of(&deltas[i]);
      const bool full = !keys || !keys[i];
      hr[i].keys = full ? nullptr : keys[i];
      hr[i].n_keys = full ? 0 : n_keys[i];
      hr[i].ctx = ctx_of(&dctxs[i]);
    }
    u64 max_run = 0;  // the fill's slices per run: a multiple of 8, each <= KFOLD_FILL_SLICE
    for (int i = 0; i < k; i++) max_run = std::max<u64>({max_run, deltas[i].n, hr[i].n_keys});
    const u64 fill_p = 8 * std::max<u64>(1, ceil_div(max_run, 8 * KFOLD_FILL_SLICE));
    if (fill_p >= (1ull << 31)) return DG_OK;
    u64* hc = h.cflat;
    hc[0] = 0;
    for (int i = 0; i < k; i++) hc[i + 1] = hc[i] + (((dotsmask >> i) & 1) ? dctxs[i].n : 0);
    KFoldArgs p{};
    p.s = rows_of(state);
    p.c0 = ctx_of(ctx);
    p.runs = (const KRun*)d.staged.runs;
    p.cflat = d.staged.cflat;
    p.sstart = d.sstart;
    p.dstart = d.dstart;
    p.tabC = d.tabC;
    p.tabP = d.tabP;
    p.flag = d.flag;
    p.dotsmask = dotsmask;
    p.dset = d.dset;
    p.dset_mask = dset_n - 1;
    p.dset_n = hc[k];
    p.k = k;
    p.allmask = allmask;
    p.T = T;
    p.fill_p = (u32)fill_p;  // the delta runs; the state's starts: kfold_fill_kernel's
                             // trailing workgroups (state_start, one wave per bucket)
    p.out = rows_out_of(out);
    p.out_ctx_node = out_ctx->node;
    p.out_ctx_cnt = out_ctx->cnt;
    p.d_counts = e->d_counts;
    HIP_TRY(hipMemcpyAsync(d.staged.runs, e->h_stage.p, d.staged_bytes, hipMemcpyHostToDevice, e->stream));
    // start tables (empty runs keep 0), VV tables (absent node = 0) and the flag; the
    // dot set's slots empty (all ones)
    HIP_TRY(hipMemsetAsync(p.sstart, 0, d.zero_bytes, e->stream));
    if (dotsmask) HIP_TRY(hipMemsetAsync(p.dset, 0xFF, dset_n * 8, e->stream));
    TRY(next_scan(e, &p.scan));
    HIP_TRY(launch_kfold(p, e->stream));
    HIP_TRY(hipMemcpyAsync(&e->h_counts[HC_KFOLD_FLAG], p.flag, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    TRY(read_counts(e));  // synchronizes; the staging buffer is free again
    u32 flag = 0;
    memcpy(&flag, &e->h_counts[HC_KFOLD_FLAG], sizeof(u32));
    if (flag & KF_PREP_FAIL) return DG_OK;
    if (flag) continue;
    out->n = e->h_counts[JC_ROWS];
    out_ctx->n = e->h_counts[JC_CTX];
    out_ctx->kind = DG_CTX_VV;
    *stepwise = false;
    return DG_OK;
  }
  return DG_OK;
}

}  // namespace

// dg_apply_deltas: passes of up to KFOLD_MAX_K deltas (each a one-pass fold), or the
// delta-by-delta fold when an input needs it.  (dg_join_deltas folds through it too.)
int apply_deltas(dg_engine* e, const dg_store* state, const dg_context* ctx, int k,
                 const dg_store* deltas, const dg_context* dctxs, const uint64_t* const* keys,
                 const uint64_t* n_keys, dg_store* out, dg_context* out_ctx) {
  if (e->apply_mode == 1 || k == 0)
    return fold_join(e, state, ctx, k, deltas, dctxs, keys, n_keys, out, out_ctx,
                     "dg_apply_deltas");
  u64 total = state->n, total_ctx = ctx->n;
  for (int s = 0; s < k; s++) {
    TRY(check_store(&deltas[s], "dg_apply_deltas delta"));
    TRY(check_ctx(&dctxs[s], "dg_apply_deltas delta ctx"));
    total += deltas[s].n;
    total_ctx += dctxs[s].n;
  }
  if (out->cap < total || out_ctx->cap < total_ctx)
    return fail(DG_E_CAPACITY, "dg_apply_deltas: output capacity too small (%llu rows, %llu ctx needed)",
                (unsigned long long)total, (unsigned long long)total_ctx);
  if (total && (!out->key || !out->val || !out->ts || !out->node || !out->cnt))
    return fail(DG_E_INVAL, "dg_apply_deltas: null output column");
  TRY(set_device(e));
  const int passes = (k + KFOLD_MAX_K - 1) / KFOLD_MAX_K;
  dg_store buf[2];
  dg_context bufc[2];
  if (passes > 1) TRY(fold_buffers(e, total, total_ctx, buf, bufc));
  dg_store acc = *state;
  dg_context acc_ctx = *ctx;
  for (int q = 0; q < passes; q++) {
    const int i0 = q * KFOLD_MAX_K, kq = std::min(KFOLD_MAX_K, k - i0);
    dg_store* dst = (q == passes - 1) ? out : &buf[q & 1];
    dg_context* dstc = (q == passes - 1) ? out_ctx : &bufc[q & 1];
    bool stepwise = false;
    TRY(kfold_pass(e, &acc, &acc_ctx, kq, deltas + i0, dctxs + i0, keys ? keys + i0 : nullptr,
                   n_keys ? n_keys + i0 : nullptr, dst, dstc, &stepwise));
    if (stepwise && e->apply_mode == 2)
      return fail(DG_E_INVAL, "dg_apply_deltas: one-pass fold not applicable to this input");
    if (stepwise)  // from the original state: fold_join reuses the ping-pong buffers
      return fold_join(e, state, ctx, k, deltas, dctxs, keys, n_keys, out, out_ctx,
                       "dg_apply_deltas");
    acc = *dst;
    acc_ctx = *dstc;
  }
  return DG_OK;
}

extern "C" {

int dg_joink(dg_engine* e, int k, const dg_store* stores, const dg_context* ctxs, dg_store* out,
             dg_context* out_ctx) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (k <= 0 || !stores || !ctxs || !out || !out_ctx) return fail(DG_E_INVAL, "dg_joink: bad args");
  TRY(check_store(&stores[0], "dg_joink store"));
  TRY(check_ctx(&ctxs[0], "dg_joink ctx"));
  TRY(settle(e));
  return fold_join(e, &stores[0], &ctxs[0], k - 1, stores + 1, ctxs + 1, nullptr, nullptr, out,
                   out_ctx, "dg_joink");
}

int dg_apply_deltas(dg_engine* e, const dg_store* state, const dg_context* ctx, int k,
                    const dg_store* deltas, const dg_context* dctxs,
                    const uint64_t* const* keys, const uint64_t* n_keys, dg_store* out,
                    dg_context* out_ctx) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (k < 0 || (k > 0 && (!deltas || !dctxs)) || !out || !out_ctx)
    return fail(DG_E_INVAL, "dg_apply_deltas: bad args");
  TRY(check_store(state, "dg_apply_deltas state"));
  TRY(check_ctx(ctx, "dg_apply_deltas ctx"));
  if (keys && !n_keys) return fail(DG_E_INVAL, "dg_apply_deltas: keys without n_keys");
  TRY(settle(e));
  return apply_deltas(e, state, ctx, k, deltas, dctxs, keys, n_keys, out, out_ctx);
}

}  // extern "C"
