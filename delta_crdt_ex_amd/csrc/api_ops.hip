// api_ops.hip — the rest of the C-ABI: take, mutate, context union and compress, reads,
// remap, mark, sort, and the memory and store calls.
#include "dg_engine.h"

extern "C" {

int dg_take_keys(dg_engine* e, const dg_store* s, const uint64_t* keys, uint64_t n_keys,
                 dg_store* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(s, "dg_take_keys"));
  if (!out || (n_keys && !keys)) return fail(DG_E_INVAL, "dg_take_keys: null argument");
  if (out->cap && (!out->key || !out->val || !out->ts || !out->node || !out->cnt))
    return fail(DG_E_INVAL, "dg_take_keys: null output column");
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_state(e, take_tiles(n_keys) + 1));
  Scan sc;
  TRY(next_scan(e, &sc));
  HIP_TRY(launch_take_keys(rows_of(s), keys, n_keys, rows_out_of(out), out->cap, sc, e->d_counts,
                           e->stream));
  TRY(read_counts(e));
  out->n = e->h_counts[JC_ROWS];
  if (out->n > out->cap)
    return fail(DG_E_CAPACITY, "dg_take_keys: %llu rows > cap %llu", (unsigned long long)out->n,
                (unsigned long long)out->cap);
  return DG_OK;
}

static int mutate_batch_impl(dg_engine* e, const dg_store* state, const dg_context* ctx, uint32_t node,
                             uint64_t m, const uint8_t* kind, const uint64_t* key, const uint64_t* val,
                             const int64_t* ts, const uint64_t* add_rank, uint64_t n_adds, dg_store* delta,
                             dg_context* delta_dots, uint64_t* keys_out, uint64_t keys_cap,
                             uint64_t* n_keys_out, bool sync) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(state, "dg_mutate_batch state"));
  TRY(check_ctx(ctx, "dg_mutate_batch ctx"));
  if (ctx->kind != DG_CTX_VV)
    return fail(DG_E_INVAL, "dg_mutate_batch: the state's context must be a version vector "
                            "(compress_dots/1 it first)");
  if (!delta || !delta_dots || !n_keys_out || (m && (!kind || !key || !val || !ts || !add_rank)))
    return fail(DG_E_INVAL, "dg_mutate_batch: null argument");
  if (n_adds > m) return fail(DG_E_INVAL, "dg_mutate_batch: n_adds > m");
  TRY(set_device(e));
  TRY(settle(e));
  const u64 nt = mutate_tiles(m);
  TRY(ensure_state(e, 6 * nt + 2));  // raw per-tile counts and offsets
  u32* err = e->ticket + TK_INPUT;
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(u32), e->stream));
  HIP_TRY(launch_mutate_count(rows_of(state), ctx_of(ctx), node, kind, key, val, ts, add_rank, m,
                              e->state.as<u64>(), e->d_counts, err, e->ticket + MUT_ARRIVE, e->stream));
  TRY(read_counts(e));  // (the counts and the order flag in one wait)
  const u64 n_keys = e->h_counts[MC_KEYS], n_rows = e->h_counts[MC_ROWS], n_sdots = e->h_counts[MC_SDOTS];
  if (e->h_ticket[TK_INPUT] & 1u) return fail(DG_E_ORDER, "dg_mutate_batch: ops are not sorted by key");
  const u64 n_dots = n_sdots + n_adds;
  if (keys_cap < n_keys || delta->cap < n_rows || delta_dots->cap < n_dots)
    return fail(DG_E_CAPACITY,
                "dg_mutate_batch: needs %llu keys, %llu delta rows, %llu context dots",
                (unsigned long long)n_keys, (unsigned long long)n_rows, (unsigned long long)n_dots);
  if ((n_keys && !keys_out) || (n_rows && (!delta->key || !delta->val || !delta->ts ||
                                           !delta->node || !delta->cnt)) ||
      (n_dots && (!delta_dots->node || !delta_dots->cnt)))
    return fail(DG_E_INVAL, "dg_mutate_batch: null output column");
  const size_t sort_b = round_up(mutate_sort_tmp_bytes(n_dots), 256);
  MutateScratch t;
  TRY(carve(e, &e->tmp, [&](Arena& a) { return mutate_layout(a, n_dots, sort_b); }, &t));
  HIP_TRY(launch_mutate_write(rows_of(state), ctx_of(ctx), node, kind, key, val, ts, add_rank, m,
                              e->state.as<u64>(), keys_out, rows_out_of(delta), t.dnode, t.dcnt, err, e->stream));
  HIP_TRY(launch_mutate_dots(ctx_of(ctx), node, n_adds, n_sdots, t.dnode, t.dcnt, t.tnode, t.tcnt, t.sort_tmp,
                             sort_b, delta_dots->node, delta_dots->cnt, e->stream));
  if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
  delta->n = n_rows;
  delta_dots->n = n_dots;
  delta_dots->kind = DG_CTX_DOTS;
  *n_keys_out = n_keys;
  return DG_OK;
}

int dg_mutate_batch(dg_engine* e, const dg_store* state, const dg_context* ctx, uint32_t node,
                    uint64_t m, const uint8_t* kind, const uint64_t* key, const uint64_t* val,
                    const int64_t* ts, const uint64_t* add_rank, uint64_t n_adds, dg_store* delta,
                    dg_context* delta_dots, uint64_t* keys_out, uint64_t keys_cap,
                    uint64_t* n_keys_out) {
  return mutate_batch_impl(e, state, ctx, node, m, kind, key, val, ts, add_rank, n_adds, delta, delta_dots,
                           keys_out, keys_cap, n_keys_out, true);
}

int dg_mutate_batch_async(dg_engine* e, const dg_store* state, const dg_context* ctx, uint32_t node,
                          uint64_t m, const uint8_t* kind, const uint64_t* key, const uint64_t* val,
                          const int64_t* ts, const uint64_t* add_rank, uint64_t n_adds, dg_store* delta,
                          dg_context* delta_dots, uint64_t* keys_out, uint64_t keys_cap,
                          uint64_t* n_keys_out) {
  return mutate_batch_impl(e, state, ctx, node, m, kind, key, val, ts, add_rank, n_adds, delta, delta_dots,
                           keys_out, keys_cap, n_keys_out, false);
}

int dg_context_union(dg_engine* e, const dg_context* a, const dg_context* b, dg_context* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_ctx(a, "dg_context_union a"));
  TRY(check_ctx(b, "dg_context_union b"));
  if (!out) return fail(DG_E_INVAL, "dg_context_union: null out");
  if (out->cap < a->n + b->n) return fail(DG_E_CAPACITY, "dg_context_union: out cap too small");
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_tmp(e, ctx_union_tmp_bytes(a->n, b->n)));
  HIP_TRY(launch_ctx_union(ctx_of(a), ctx_of(b), out->node, out->cnt, e->d_counts + JC_CTX, e->tmp.p,
                           e->stream));
  TRY(read_counts(e));
  out->n = e->h_counts[JC_CTX];
  out->kind = (a->kind == DG_CTX_DOTS && b->kind == DG_CTX_DOTS) ? DG_CTX_DOTS : DG_CTX_VV;
  return DG_OK;
}

int dg_compress_dots(dg_engine* e, const dg_context* dots, dg_context* out_vv) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_ctx(dots, "dg_compress_dots"));
  if (dots->kind != DG_CTX_DOTS)
    return fail(DG_E_CLAUSE,
                "no function clause matching in DeltaCrdt.AWLWWMap.Dots.compress/1 "
                "(context is already a version vector; aw_lww_map.ex:13)");
  dg_context empty;
  memset(&empty, 0, sizeof empty);
  empty.kind = DG_CTX_VV;
  return dg_context_union(e, &empty, dots, out_vv);
}

int dg_read_lww(dg_engine* e, const dg_store* s, const uint64_t* keys, uint64_t n_keys,
                uint64_t* out_key, uint64_t* out_val, uint64_t cap, uint64_t* n_out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(s, "dg_read_lww"));
  if (!n_out || (s->n && (!out_key || !out_val))) return fail(DG_E_INVAL, "dg_read_lww: null output");
  if (keys == nullptr && n_keys != 0) return fail(DG_E_INVAL, "dg_read_lww: keys NULL with n_keys>0");
  u64 need = keys ? std::min<u64>(n_keys, s->n) : s->n;
  if (cap < need)
    return fail(DG_E_CAPACITY, "dg_read_lww: cap %llu < %llu", (unsigned long long)cap,
                (unsigned long long)need);
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_state(e, 2 * seg_tiles(s->n) + 2));  // raw per-tile counts and offsets
  HIP_TRY(launch_read_lww(rows_of(s), keys, keys ? n_keys : 0, out_key, out_val, e->state.as<u64>(),
                          e->d_counts, e->stream));
  TRY(read_counts(e));
  *n_out = e->h_counts[JC_ROWS];
  return DG_OK;
}

int dg_remap_values(dg_engine* e, dg_store* s, const uint64_t* old_ids, const uint64_t* new_ids,
                    uint64_t n_ids) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(s, "dg_remap_values"));
  if (n_ids && (!old_ids || !new_ids)) return fail(DG_E_INVAL, "dg_remap_values: null id table");
  if (s->n == 0) return DG_OK;
  TRY(set_device(e));
  TRY(settle(e));
  HIP_TRY(hipMemsetAsync(e->ticket + TK_INPUT, 0, sizeof(u32), e->stream));
  HIP_TRY(launch_remap_values(s->val, s->n, old_ids, new_ids, n_ids, e->ticket + TK_INPUT, e->stream));
  TRY(sync_words(e));
  if (e->h_ticket[TK_INPUT]) return fail(DG_E_INVAL, "dg_remap_values: a row's value id is not in old_ids");
  return DG_OK;
}

static_assert(DG_MARK_COL_KEY == DG_COL_KEY && DG_MARK_COL_VAL == DG_COL_VAL, "deltagpu.h's columns are the kernels'");

int dg_mark_ids(dg_engine* e, const dg_store* stores, uint64_t n_stores, int column, const uint64_t* ids,
                uint64_t n_ids, uint8_t* used, uint64_t* n_used, uint64_t* n_unknown) {
  if (column != DG_COL_KEY && column != DG_COL_VAL) return fail(DG_E_INVAL, "dg_mark_ids: bad column %d", column);
  if (n_stores && !stores) return fail(DG_E_INVAL, "dg_mark_ids: null stores with n_stores=%llu",
                                       (unsigned long long)n_stores);
  if (n_ids && (!ids || !used)) return fail(DG_E_INVAL, "dg_mark_ids: null id table or flags");
  if (!n_used) return fail(DG_E_INVAL, "dg_mark_ids: null n_used");
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (n_ids >= (1ull << 40) || n_stores >= (1ull << 24))
    return fail(DG_E_INVAL, "dg_mark_ids: more than 2^40 - 1 ids or 2^24 - 1 stores");
  for (u64 i = 0; i < n_stores; i++) TRY(check_store(&stores[i], "dg_mark_ids"));
  TRY(set_device(e));
  TRY(settle(e));
  // the stores' columns as one tile sequence: descriptors staged in pinned memory, copied on
  // the engine stream ahead of the kernels (one launch chain whatever n_stores is)
  TRY(ensure_stage(e, std::max<size_t>((n_stores + 1) * sizeof(MarkSeg), 8 * 256 * sizeof(u32))));
  MarkScratch mk;
  TRY(carve(e, &e->tmp, [&](Arena& a) {
    return mark_layout(a, n_stores, sizeof(MarkSeg), mark_bitmap_words(n_ids), MARK_LDS_IDS);
  }, &mk));
  MarkSeg* hs = e->h_stage.as<MarkSeg>();
  u64 tiles = 0;
  for (u64 i = 0; i < n_stores; i++) tiles += mark_tiles(stores[i].n, MARK_TILE_SMALL);
  const u64 tile_rows = column == DG_COL_KEY && tiles <= MARK_SMALL_TILES ? MARK_TILE_SMALL : MARK_TILE;
  tiles = 0;
  for (u64 i = 0; i < n_stores; i++) {
    hs[i].col = column == DG_COL_KEY ? stores[i].key : stores[i].val;
    hs[i].n = stores[i].n;
    hs[i].tile0 = tiles;
    tiles += mark_tiles(stores[i].n, tile_rows);
  }
  hs[n_stores] = MarkSeg{nullptr, 0, tiles};
  MarkSeg* ds = (MarkSeg*)mk.segs;
  if (tiles)
    HIP_TRY(hipMemcpyAsync(ds, hs, (n_stores + 1) * sizeof(MarkSeg), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(launch_mark_ids(ds, n_stores + 1, tiles, tile_rows, column, mark_mode(column, n_ids), ids, n_ids, mk.bitmap, mk.samples, used,
                          e->d_counts, e->ticket + TK_INPUT, e->stream));
  TRY(read_counts(e));
  if (e->h_ticket[TK_INPUT]) return fail(DG_E_ORDER, "dg_mark_ids: the id table is not strictly ascending");
  *n_used = e->h_counts[MK_USED];
  if (n_unknown) *n_unknown = e->h_counts[MK_UNKNOWN];
  return DG_OK;
}

int dg_sort_store(dg_engine* e, const dg_store* in, dg_store* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(in, "dg_sort_store"));
  if (!out) return fail(DG_E_INVAL, "dg_sort_store: null out");
  if (out->cap < in->n)
    return fail(DG_E_CAPACITY, "dg_sort_store: out cap %llu < %llu rows", (unsigned long long)out->cap,
                (unsigned long long)in->n);
  if (in->n && (!out->key || !out->val || !out->ts || !out->node || !out->cnt))
    return fail(DG_E_INVAL, "dg_sort_store: null output column");
  if (in->n >= (1ull << 32)) return fail(DG_E_INVAL, "dg_sort_store: more than 2^32 - 1 rows");
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_tmp(e, sort_tmp_bytes(in->n)));
  TRY(ensure_stage(e, 8 * 256 * sizeof(u32)));
  HIP_TRY(launch_sort_store(rows_of(in), rows_out_of(out), e->tmp.p, e->h_stage.as<u32>(), e->d_counts,
                            e->stream));
  TRY(read_counts(e));
  out->n = e->h_counts[JC_ROWS];
  return DG_OK;
}

int dg_sort_context(dg_engine* e, const dg_context* in, dg_context* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_ctx(in, "dg_sort_context"));
  if (!out) return fail(DG_E_INVAL, "dg_sort_context: null out");
  if (out->cap < in->n) return fail(DG_E_CAPACITY, "dg_sort_context: out cap too small");
  if (in->n && (!out->node || !out->cnt)) return fail(DG_E_INVAL, "dg_sort_context: null output");
  if (in->n >= (1ull << 32)) return fail(DG_E_INVAL, "dg_sort_context: more than 2^32 - 1 entries");
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_tmp(e, sort_tmp_bytes(in->n)));
  TRY(ensure_stage(e, 8 * 256 * sizeof(u32)));
  HIP_TRY(launch_sort_context(in->kind, in->node, in->cnt, in->n, out->node, out->cnt, e->tmp.p,
                              e->h_stage.as<u32>(), e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  out->n = in->n;
  out->kind = in->kind;
  return DG_OK;
}

// ---- device buffers
int dg_buffer_alloc(dg_engine* e, uint64_t bytes, void** p) {
  if (!e || !p) return fail(DG_E_INVAL, "dg_buffer_alloc: null argument");
  *p = nullptr;
  TRY(set_device(e));
  if (bytes == 0) return DG_OK;
  if (hipMalloc(p, bytes) != hipSuccess) {
    *p = nullptr;
    return fail(DG_E_NOMEM, "hipMalloc of %llu bytes failed", (unsigned long long)bytes);
  }
  return DG_OK;
}

int dg_buffer_free(dg_engine* e, void* p) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!p) return DG_OK;
  TRY(set_device(e));
  HIP_TRY(hipStreamSynchronize(e->stream));  // no kernel of this engine still uses it
  HIP_TRY(hipFree(p));
  return DG_OK;
}

int dg_copy_to_device(dg_engine* e, void* dst, const void* src, uint64_t bytes) {
  if (!e || (bytes && (!dst || !src))) return fail(DG_E_INVAL, "dg_copy_to_device: null argument");
  if (!bytes) return DG_OK;
  TRY(set_device(e));
  // (hipMemcpyDefault: the source may be device memory too -- a device-to-device copy)
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DG_OK;
}

int dg_copy_to_host(dg_engine* e, void* dst, const void* src, uint64_t bytes) {
  if (!e || (bytes && (!dst || !src))) return fail(DG_E_INVAL, "dg_copy_to_host: null argument");
  if (!bytes) return DG_OK;
  TRY(set_device(e));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return DG_OK;
}

int dg_copy_async(dg_engine* e, void* dst, const void* src, uint64_t bytes) {
  if (!e || (bytes && (!dst || !src))) return fail(DG_E_INVAL, "dg_copy_async: null argument");
  if (!bytes) return DG_OK;
  TRY(set_device(e));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
  return DG_OK;
}

int dg_host_alloc(dg_engine* e, uint64_t bytes, void** p) {
  if (!e || !p) return fail(DG_E_INVAL, "dg_host_alloc: null argument");
  *p = nullptr;
  TRY(set_device(e));
  if (bytes == 0) return DG_OK;
  if (hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    *p = nullptr;
    return fail(DG_E_NOMEM, "hipHostMalloc of %llu bytes failed", (unsigned long long)bytes);
  }
  return DG_OK;
}

int dg_host_free(dg_engine* e, void* p) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!p) return DG_OK;
  TRY(set_device(e));
  HIP_TRY(hipStreamSynchronize(e->stream));  // no copy of this engine still reads or writes it
  HIP_TRY(hipHostFree(p));
  return DG_OK;
}

int dg_store_alloc(dg_engine* e, uint64_t cap, dg_store* s) {
  if (!e || !s) return fail(DG_E_INVAL, "dg_store_alloc: null argument");
  memset(s, 0, sizeof *s);
  const uint64_t c = cap ? cap : 1;
  void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const uint64_t w[5] = {8, 8, 8, 4, 8};
  for (int i = 0; i < 5; i++) {
    int rc = dg_buffer_alloc(e, c * w[i], &p[i]);
    if (rc != DG_OK) {
      for (int j = 0; j < i; j++) hipFree(p[j]);
      return rc;
    }
  }
  s->key = (uint64_t*)p[0];
  s->val = (uint64_t*)p[1];
  s->ts = (int64_t*)p[2];
  s->node = (uint32_t*)p[3];
  s->cnt = (uint64_t*)p[4];
  s->cap = cap;
  return DG_OK;
}

int dg_store_free(dg_engine* e, dg_store* s) {
  if (!e || !s) return fail(DG_E_INVAL, "dg_store_free: null argument");
  void* p[5] = {s->key, s->val, s->ts, s->node, s->cnt};
  for (int i = 0; i < 5; i++) TRY(dg_buffer_free(e, p[i]));
  memset(s, 0, sizeof *s);
  return DG_OK;
}

int dg_store_upload(dg_engine* e, const dg_store* host, dg_store* dev) {
  if (!e || !host || !dev) return fail(DG_E_INVAL, "dg_store_upload: null argument");
  if (dev->cap < host->n) return fail(DG_E_CAPACITY, "dg_store_upload: device cap too small");
  TRY(set_device(e));
  const uint64_t n = host->n;
  if (n) {
    TRY(copy_rows(e, dev, host, n, hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  dev->n = n;
  return DG_OK;
}

int dg_store_download(dg_engine* e, const dg_store* dev, dg_store* host) {
  if (!e || !host || !dev) return fail(DG_E_INVAL, "dg_store_download: null argument");
  if (host->cap < dev->n) return fail(DG_E_CAPACITY, "dg_store_download: host cap too small");
  TRY(set_device(e));
  const uint64_t n = dev->n;
  if (n) {
    TRY(copy_rows(e, host, dev, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  host->n = n;
  return DG_OK;
}

int dg_context_alloc(dg_engine* e, uint64_t cap, dg_context* c) {
  if (!e || !c) return fail(DG_E_INVAL, "dg_context_alloc: null argument");
  memset(c, 0, sizeof *c);
  void *pn = nullptr, *pc = nullptr;
  TRY(dg_buffer_alloc(e, (cap ? cap : 1) * 4, &pn));
  int rc = dg_buffer_alloc(e, (cap ? cap : 1) * 8, &pc);
  if (rc != DG_OK) {
    hipFree(pn);
    return rc;
  }
  c->node = (uint32_t*)pn;
  c->cnt = (uint64_t*)pc;
  c->cap = cap;
  return DG_OK;
}

int dg_context_free(dg_engine* e, dg_context* c) {
  if (!e || !c) return fail(DG_E_INVAL, "dg_context_free: null argument");
  TRY(dg_buffer_free(e, c->node));
  TRY(dg_buffer_free(e, c->cnt));
  memset(c, 0, sizeof *c);
  return DG_OK;
}

int dg_context_upload(dg_engine* e, const dg_context* host, dg_context* dev) {
  if (!e || !host || !dev) return fail(DG_E_INVAL, "dg_context_upload: null argument");
  if (dev->cap < host->n) return fail(DG_E_CAPACITY, "dg_context_upload: device cap too small");
  TRY(dg_copy_to_device(e, dev->node, host->node, host->n * 4));
  TRY(dg_copy_to_device(e, dev->cnt, host->cnt, host->n * 8));
  dev->n = host->n;
  dev->kind = host->kind;
  return DG_OK;
}

int dg_context_download(dg_engine* e, const dg_context* dev, dg_context* host) {
  if (!e || !host || !dev) return fail(DG_E_INVAL, "dg_context_download: null argument");
  if (host->cap < dev->n) return fail(DG_E_CAPACITY, "dg_context_download: host cap too small");
  TRY(dg_copy_to_host(e, host->node, dev->node, dev->n * 4));
  TRY(dg_copy_to_host(e, host->cnt, dev->cnt, dev->n * 8));
  host->n = dev->n;
  host->kind = dev->kind;
  return DG_OK;
}


}  // extern "C"
