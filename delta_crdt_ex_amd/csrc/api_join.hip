// api_join.hip — the joins of the C-ABI: dg_join2, its asynchronous and change-reporting
// forms, and the sparse keyed join as a splice.
#include "dg_engine.h"

// chg (optional): the join also records its change events (dg_join2_changes); *chg
// receives their scratch for launch_join2_changes.
int join2_enqueue(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
                  const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
                  dg_context* out_ctx, uint64_t* d_counts, void** chg, bool force_two_pass) {
  TRY(check_store(a, "dg_join2 a"));
  TRY(check_store(b, "dg_join2 b"));
  TRY(check_ctx(ca, "dg_join2 ca"));
  TRY(check_ctx(cb, "dg_join2 cb"));
  if (!out || !out_ctx || !d_counts) return fail(DG_E_INVAL, "dg_join2: null output");
  if (keys == nullptr && n_keys != 0) return fail(DG_E_INVAL, "dg_join2: keys NULL with n_keys>0");
  if (out->cap < a->n + b->n)
    return fail(DG_E_CAPACITY, "dg_join2: out cap %llu < %llu rows in", (unsigned long long)out->cap,
                (unsigned long long)(a->n + b->n));
  if (out_ctx->cap < ca->n + cb->n)
    return fail(DG_E_CAPACITY, "dg_join2: out_ctx cap %llu < %llu", (unsigned long long)out_ctx->cap,
                (unsigned long long)(ca->n + cb->n));
  if (a->n + b->n && (!out->key || !out->val || !out->ts || !out->node || !out->cnt))
    return fail(DG_E_INVAL, "dg_join2: null output column");
  TRY(set_device(e));
  const u64 tiles = join2_tiles(a->n, b->n), tiles_cap = join2_tiles_cap(a->n, b->n);
  Arena state;  // (measured: launch_join2 carves it)
  join_state_layout(state, tiles_cap);
  TRY(ensure_state(e, state.off / sizeof(u64)));
  const bool two_pass = (force_two_pass || e->join_mode == JOIN_TWO_PASS) && !chg;  // changes: single pass
  if (!two_pass) TRY(ensure_counts(e, tiles_cap));
  JoinScratch js;
  TRY(carve(e, &e->tmp, [&](Arena& m) {
    return join_layout(m, ctx_union_tmp_bytes(ca->n, cb->n),
                       two_pass ? measured([&](Arena& x) { pass_layout(x, tiles, JOIN_TILE); }) : 0,
                       chg ? measured([&](Arena& x) { chg_layout(x, tiles, JOIN_TILE); }) : 0);
  }, &js));
  if (chg) *chg = js.chg;
  Scan sc;
  TRY(next_scan(e, &sc));
  hipStream_t st = e->stream;
  hipStream_t ps = two_pass ? nullptr : shared_join_stream(e);
  if (ps) {
    HIP_TRY(hipEventRecord(e->ev_in, e->stream));
    HIP_TRY(hipStreamWaitEvent(ps, e->ev_in, 0));
    st = ps;
  }
  HIP_TRY(launch_join2(rows_of(a), ctx_of(ca), rows_of(b), ctx_of(cb), keys, keys ? n_keys : 0,
                       rows_out_of(out), out_ctx->node, out_ctx->cnt, js.ctx, js.pass,
                       two_pass ? JOIN_TWO_PASS : JOIN_SINGLE_PASS, sc, e->join_workers, d_counts, st, js.chg,
                       e->join_stagger));
  if (ps) {
    HIP_TRY(hipEventRecord(e->ev_out, ps));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_out, 0));
  }
  out_ctx->kind = (ca->kind == DG_CTX_DOTS && cb->kind == DG_CTX_DOTS) ? DG_CTX_DOTS : DG_CTX_VV;
  return DG_OK;
}

// A keyed join whose delta and keyset are small against the state (CausalCrdt's sync
// deltas, causal_crdt.ex:383-384) as a splice (csrc/splice.hip): the state's rows of the
// keyset are taken out, joined with the delta on the join kernels, and the output is
// written in one streaming pass (the untouched rows moved, the joined keys' rows in the
// holes).  *done = false (and nothing of the caller's changed) when the splice does not
// apply: the delta holds a key outside the keyset (its right-biased carry would replace
// state rows the splice keeps), the taken rows exceed their bound, or the join grid
// aborted; the caller then runs the full join.  Synchronous (two host syncs).
// (the splice moves rows in 16-byte pairs: the state's and the output's 8-byte columns
// must be 16-byte aligned, their node columns 8-byte aligned)
bool splice_wanted(const dg_engine* e, const dg_store* a, const dg_store* b, const uint64_t* keys,
                   uint64_t n_keys, const dg_store* out) {
  return e->splice && keys && n_keys > 0 && (n_keys + b->n) * 8 <= a->n && out &&
         pair_aligned(a->key, a->val, a->ts, a->node, a->cnt) &&
         pair_aligned(out->key, out->val, out->ts, out->node, out->cnt);
}

// Phase 1: take the state's rows of the keyset (with the per-key index) and check that
// every key of the delta is in the keyset.  *ok = false: the splice does not apply (the
// full join does).  One host sync.
int splice_take(dg_engine* e, const dg_store* a, const dg_store* b, const uint64_t* keys,
                uint64_t n_keys, u64 uctx_cap, Splice* w, bool* ok) {
  *ok = false;
  const u64 cap_k = std::min<u64>(a->n, 16 * n_keys + 4096);  // taken rows: a few per key
  const u64 cap_e = cap_k + b->n;
  SpliceScratch s;
  TRY(carve(e, &e->spl, [&](Arena& m) { return splice_layout(m, cap_k, cap_e, n_keys, splice_tiles(a->n), uctx_cap); },
            &s));
  w->ak = s.ak;
  w->ed = s.ed;
  w->uctx = s.uctx;
  SpliceArgs& sp = w->sp;
  sp = SpliceArgs{};
  sp.a_lo = s.idx.a_lo;
  sp.a_off = s.idx.a_off;
  sp.end = s.idx.end;
  sp.shift = s.idx.shift;
  sp.gap = s.idx.gap;
  sp.tile_u0 = s.tile_u0;
  sp.moved = (u32*)(e->d_counts + SC_MOVED);  // zeroed with n_ak and bad below
  TRY(ensure_state(e, take_tiles(n_keys) + 2));
  Scan sc;
  TRY(next_scan(e, &sc));
  static_assert(SC_BAD == SC_TAKEN + 1 && SC_MOVED == SC_TAKEN + 2, "zeroed as one range");
  HIP_TRY(hipMemsetAsync(e->d_counts + SC_TAKEN, 0, 3 * sizeof(u64), e->stream));
  // the keyset's rows: one search per key, or -- once the keys are dense enough that the
  // searches' scattered lines outweigh reading every key -- one streaming pass over the
  // state's keys (the located ranges go through `end`, which the index overwrites later).
  // At 1 key in 100 rows (config 4) both take 60 us for 12.5M rows; the searches grow
  // with the keys, the pass does not.
  u32* pre_len = nullptr;
  if (n_keys * 60 >= a->n) {
    pre_len = (u32*)sp.end;
    HIP_TRY(launch_splice_locate(rows_of(a), keys, n_keys, (u64*)sp.a_lo, pre_len, e->stream));
  }
  HIP_TRY(launch_take_keys(rows_of(a), keys, n_keys, rows_out_of(&w->ak), cap_k, sc,
                           e->d_counts + SC_TAKEN, e->stream, (u64*)sp.a_lo, (u64*)sp.a_off, pre_len));
  HIP_TRY(launch_splice_check(b->key, b->n, keys, n_keys, e->d_counts + SC_BAD, e->stream));
  TRY(read_counts(e));
  w->n_ak = e->h_counts[SC_TAKEN];
  if (e->h_counts[SC_BAD] != 0 || w->n_ak > cap_k) return DG_OK;
  w->ak.n = w->n_ak;
  sp.a = rows_of(a);
  sp.keys = keys;
  sp.nk = n_keys;
  sp.e = rows_of(&w->ed);
  sp.e.n = w->n_ak + b->n;  // a bound: the kernels read the count
  sp.d_ne = e->d_counts + JC_ROWS;
  *ok = true;
  return DG_OK;
}

// Phase 2: the edit E = join(taken rows, delta, keys) (+ its changed keys) and the index.
int splice_edit(dg_engine* e, Splice* w, const dg_context* ca, const dg_store* b,
                const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_context* out_ctx,
                bool with_changes, uint64_t* changed, uint64_t cap) {
  void* chg = nullptr;
  TRY(join2_enqueue(e, &w->ak, ca, b, cb, keys, n_keys, &w->ed, out_ctx, e->d_counts,
                    with_changes ? &chg : nullptr));
  if (with_changes)
    HIP_TRY(launch_join2_changes(w->ak.n, b->n, chg, changed, cap, e->d_counts + JC_CHANGED, e->stream));
  HIP_TRY(launch_splice_index(w->sp, e->stream));
  return DG_OK;
}

static int splice_join(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
                       const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
                       dg_context* out_ctx, bool with_changes, uint64_t* changed, uint64_t cap,
                       uint64_t* n_changed, bool* done) {
  *done = false;
  TRY(check_store(a, "dg_join2 a"));
  TRY(check_store(b, "dg_join2 b"));
  TRY(check_ctx(ca, "dg_join2 ca"));
  TRY(check_ctx(cb, "dg_join2 cb"));
  if (!out || !out_ctx) return fail(DG_E_INVAL, "dg_join2: null output");
  if (out->cap < a->n + b->n)
    return fail(DG_E_CAPACITY, "dg_join2: out cap %llu < %llu rows in", (unsigned long long)out->cap,
                (unsigned long long)(a->n + b->n));
  if (!out->key || !out->val || !out->ts || !out->node || !out->cnt)
    return fail(DG_E_INVAL, "dg_join2: null output column");
  TRY(set_device(e));
  Splice w;
  bool ok = false;
  TRY(splice_take(e, a, b, keys, n_keys, 0, &w, &ok));
  if (!ok) return DG_OK;  // the full join applies
  TRY(splice_edit(e, &w, ca, b, cb, keys, n_keys, out_ctx, with_changes, changed, cap));
  w.sp.out = rows_out_of(out);
  HIP_TRY(launch_splice_copy(w.sp, false, e->stream));
  if (read_counts(e) != DG_OK) return DG_OK;  // a grid aborted: the full join re-runs
  out->n = a->n - w.n_ak + e->h_counts[JC_ROWS];
  out_ctx->n = e->h_counts[JC_CTX];
  if (n_changed) *n_changed = e->h_counts[JC_CHANGED];
  *done = true;
  return DG_OK;
}

extern "C" {

int dg_join2_async(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
                   const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
                   dg_context* out_ctx, uint64_t* d_counts) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (e->pending.size() >= MAX_PENDING) TRY(dg_engine_sync(e));
  TRY(join2_enqueue(e, a, ca, b, cb, keys, n_keys, out, out_ctx, d_counts));
  dg_engine::Pending q{};
  q.kind = 0;
  q.a = *a;
  q.b = *b;
  q.out = *out;
  q.ca = *ca;
  q.cb = *cb;
  q.out_ctx = *out_ctx;
  q.keys = keys;
  q.n_keys = n_keys;
  q.d_counts = d_counts;
  e->pending.push_back(q);
  return DG_OK;
}

int dg_join2(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
             const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
             dg_context* out_ctx) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(settle(e));  // earlier asynchronous calls
  if (splice_wanted(e, a, b, keys, n_keys, out)) {
    bool done = false;
    TRY(splice_join(e, a, ca, b, cb, keys, n_keys, out, out_ctx, false, nullptr, 0, nullptr, &done));
    if (done) return DG_OK;
  }
  TRY(join2_enqueue(e, a, ca, b, cb, keys, n_keys, out, out_ctx, e->d_counts));
  if (read_counts(e) != DG_OK) {
    // a single-pass grid that could not become resident (another process's persistent
    // kernels on this GPU) timed out: the two-pass kernels never wait on each other
    TRY(join2_enqueue(e, a, ca, b, cb, keys, n_keys, out, out_ctx, e->d_counts, nullptr, true));
    TRY(read_counts(e));
  }
  out->n = e->h_counts[JC_ROWS];
  out_ctx->n = e->h_counts[JC_CTX];
  return DG_OK;
}

int dg_join2_changes(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
                     const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
                     dg_context* out_ctx, uint64_t* changed, uint64_t cap, uint64_t* n_changed) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!n_changed || (cap && !changed)) return fail(DG_E_INVAL, "dg_join2_changes: null output");
  TRY(settle(e));
  if (splice_wanted(e, a, b, keys, n_keys, out)) {
    bool done = false;
    TRY(splice_join(e, a, ca, b, cb, keys, n_keys, out, out_ctx, true, changed, cap, n_changed, &done));
    if (done) {
      if (*n_changed > cap)
        return fail(DG_E_CAPACITY, "dg_join2_changes: %llu changed keys > cap %llu",
                    (unsigned long long)*n_changed, (unsigned long long)cap);
      return DG_OK;
    }
  }
  auto enqueue = [&]() -> int {
    void* chg = nullptr;
    TRY(join2_enqueue(e, a, ca, b, cb, keys, n_keys, out, out_ctx, e->d_counts, &chg));
    HIP_TRY(launch_join2_changes(a->n, b->n, chg, changed, cap, e->d_counts + JC_CHANGED, e->stream));
    return DG_OK;
  };
  TRY(enqueue());
  if (read_counts(e) != DG_OK) {
    // the grid aborted (not co-resident): the change events come from the single-pass
    // kernel only, so re-run it on a small grid
    TRY(with_small_grid(e, enqueue));
    TRY(read_counts(e));
  }
  out->n = e->h_counts[JC_ROWS];
  out_ctx->n = e->h_counts[JC_CTX];
  *n_changed = e->h_counts[JC_CHANGED];
  if (*n_changed > cap)
    return fail(DG_E_CAPACITY, "dg_join2_changes: %llu changed keys > cap %llu",
                (unsigned long long)*n_changed, (unsigned long long)cap);
  return DG_OK;
}

}  // extern "C"
