// api_replay.hip — dg_replace_keysets: k journal records applied to a resident state as ONE
// splice.  The records' keys become their union with each key's winning record (replay.hip),
// the winners' rows become the edit store by take.hip's copy of located runs, and the rest is
// dg_join_delta's splice path with the per-key join left out: the take of the union's state
// rows, the index, the `moved` decision, the copy and the tree update.
#include "dg_engine.h"

namespace {

enum ReplayCount {      // e->d_counts of this path
  RC_EDIT = JC_ROWS,    // the edit's rows (take_keys_kernel over the records' rows)
  RC_SUM = 1,           // the rows of every (record, key) item (replay_check_kernel)
  RC_KEYS = 2,          // union keys (replay_scan_kernel)
  RC_TAKEN = SC_TAKEN,  // the state's rows of the union (take_keys_kernel)
  RC_MOVED = SC_MOVED,  // u32: a key's row count changes (splice_index_kernel)
};
constexpr size_t HIST8_BYTES = 8 * 256 * sizeof(u32);  // sort_fields' pinned byte counts
const char* const WHAT = "dg_replace_keysets";

}  // namespace

extern "C" {

int dg_replace_keysets(dg_engine* e, dg_store* state, uint64_t k, const uint64_t* keys_cat,
                       const uint64_t* key_off, const dg_store* rows_cat, const uint64_t* row_off,
                       dg_store* spare, dg_merkle* tree, uint64_t* n_union, int* swapped) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (!state || !spare || !n_union || !swapped) return fail(DG_E_INVAL, "%s: null argument", WHAT);
  *n_union = 0;
  *swapped = 0;
  TRY(check_store(state, "dg_replace_keysets state"));
  TRY(check_store(rows_cat, "dg_replace_keysets rows_cat"));
  if (tree) TRY(check_merkle(tree, WHAT));
  if (k && (!key_off || !row_off)) return fail(DG_E_INVAL, "%s: null offsets with k > 0", WHAT);
  if (k >= (1ull << 32)) return fail(DG_E_INVAL, "%s: more than 2^32 - 1 records", WHAT);
  if (k == 0) {
    if (rows_cat->n) return fail(DG_E_INVAL, "%s: %llu rows and no record", WHAT, (unsigned long long)rows_cat->n);
    return DG_OK;
  }
  if (spare->cap < state->n + rows_cat->n)
    return fail(DG_E_CAPACITY, "%s: spare cap %llu < %llu rows in", WHAT, (unsigned long long)spare->cap,
                (unsigned long long)(state->n + rows_cat->n));
  if (state->cap < state->n) return fail(DG_E_INVAL, "%s: state cap %llu < n %llu", WHAT,
                                         (unsigned long long)state->cap, (unsigned long long)state->n);
  if ((state->n && !pair_aligned(state->key, state->val, state->ts, state->node, state->cnt)) ||
      !spare->key || !spare->val || !spare->ts || !spare->node || !spare->cnt ||
      !pair_aligned(spare->key, spare->val, spare->ts, spare->node, spare->cnt))
    return fail(DG_E_INVAL, "%s: state and spare columns must be 16-byte aligned (dg_store_alloc)", WHAT);
  TRY(set_device(e));
  TRY(settle(e));
  // the two offset tables come home first: they size everything, and the kernels' searches
  // rely on them (ascending, from 0 to the item and row totals)
  TRY(ensure_stage(e, HIST8_BYTES + 2 * (size_t)(k + 1) * sizeof(u64)));
  u32* h_hist8 = e->h_stage.as<u32>();
  u64* h_koff = (u64*)(e->h_stage.as<char>() + HIST8_BYTES);
  u64* h_roff = h_koff + (k + 1);
  HIP_TRY(hipMemcpyAsync(h_koff, key_off, (k + 1) * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(h_roff, row_off, (k + 1) * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (h_koff[0] != 0 || h_roff[0] != 0) return fail(DG_E_INVAL, "%s: offsets do not start at 0", WHAT);
  for (u64 j = 0; j < k; j++)
    if (h_koff[j] > h_koff[j + 1] || h_roff[j] > h_roff[j + 1])
      return fail(DG_E_INVAL, "%s: offsets of record %llu descend", WHAT, (unsigned long long)j);
  const u64 m = h_koff[k];
  if (h_roff[k] != rows_cat->n)
    return fail(DG_E_INVAL, "%s: row offsets end at %llu, rows_cat holds %llu", WHAT,
                (unsigned long long)h_roff[k], (unsigned long long)rows_cat->n);
  if (m >= (1ull << 32)) return fail(DG_E_INVAL, "%s: more than 2^32 - 1 keys in all", WHAT);
  if (m && !keys_cat) return fail(DG_E_INVAL, "%s: keys_cat NULL with keys", WHAT);
  if (m == 0) {  // an empty union: nothing to replace (rows without a key: outside their keyset)
    if (rows_cat->n) return fail(DG_E_INVAL, "%s: a row whose key is not in its record's keyset", WHAT);
    return DG_OK;
  }
  ReplayScratch r;
  TRY(carve(e, &e->rpl, [&](Arena& a) { return replay_layout(a, m, replay_tiles(m), sort_tmp_bytes(m)); }, &r));
  // 1. the checks and the per-item runs; nothing but scratch is written before they are read
  u32* err = e->ticket + TK_INPUT;
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(u32), e->stream));
  HIP_TRY(hipMemsetAsync(e->d_counts, 0, 8 * sizeof(u64), e->stream));
  ReplayArgs p{};
  p.keys_cat = keys_cat;
  p.key_off = key_off;
  p.rows = rows_of(rows_cat);
  p.row_off = row_off;
  p.k = k;
  p.m = m;
  p.item_lo = r.item_lo;
  p.item_len = r.item_len;
  p.d_sum = e->d_counts + RC_SUM;
  p.err = err;
  HIP_TRY(launch_replay_check(p, e->stream));
  TRY(read_counts(e));
  if (const u32 bits = e->h_ticket[TK_INPUT]) {
    HIP_TRY(hipMemsetAsync(err, 0, sizeof(u32), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (bits & RP_ERR_KEYS) return fail(DG_E_ORDER, "%s: a keyset is not strictly ascending", WHAT);
    return fail(DG_E_ORDER, "%s: a row segment is not in store order", WHAT);
  }
  if (e->h_counts[RC_SUM] != rows_cat->n)
    return fail(DG_E_INVAL, "%s: a row whose key is not in its record's keyset (%llu of %llu rows are)", WHAT,
                (unsigned long long)e->h_counts[RC_SUM], (unsigned long long)rows_cat->n);
  // 2. the union and each key's winner
  const SortField f{keys_cat, 8, 0};
  u32* idx = nullptr;
  HIP_TRY(sort_fields(&f, 1, m, r.sort_tmp, &idx, h_hist8, e->stream));
  HIP_TRY(launch_replay_union(keys_cat, idx, m, r.item_lo, r.item_len, r.tile_cnt, r.tile_off, r.ukeys, r.u_lo,
                              r.u_len, e->d_counts + RC_KEYS, e->stream));
  TRY(read_counts(e));
  const u64 nu = e->h_counts[RC_KEYS];
  // 3. the splice: the state's rows of the union out (ak), the winners' rows in key order (the
  // edit E), the index and its `moved` word.  The taken rows are bounded by a guess; a state
  // with more rows per key than that takes again at the count the first take reported.
  const u64 a_tiles = splice_tiles(state->n);
  TRY(ensure_state(e, take_tiles(nu) + 2));
  u64 cap_k = std::min<u64>(state->n, 16 * nu + 4096);
  SpliceScratch s;
  SpliceArgs sp;
  u64 n_ak = 0, n_e = 0;
  for (int attempt = 0;; attempt++) {
    TRY(carve(e, &e->spl, [&](Arena& a) { return splice_layout(a, cap_k, rows_cat->n, nu, a_tiles, 0); }, &s));
    sp = SpliceArgs{};
    sp.a = rows_of(state);
    sp.keys = r.ukeys;
    sp.nk = nu;
    sp.a_lo = s.idx.a_lo;
    sp.a_off = s.idx.a_off;
    sp.end = s.idx.end;
    sp.shift = s.idx.shift;
    sp.gap = s.idx.gap;
    sp.tile_u0 = s.tile_u0;
    sp.moved = (u32*)(e->d_counts + RC_MOVED);
    sp.e = rows_of(&s.ed);
    sp.e.n = rows_cat->n;  // a bound: the kernels read the count
    sp.d_ne = e->d_counts + RC_EDIT;
    static_assert(SC_MOVED == SC_TAKEN + 2, "zeroed as one range");
    HIP_TRY(hipMemsetAsync(e->d_counts + SC_TAKEN, 0, 3 * sizeof(u64), e->stream));
    Scan sc;
    TRY(next_scan(e, &sc));
    HIP_TRY(launch_take_keys(rows_of(state), r.ukeys, nu, rows_out_of(&s.ak), cap_k, sc, e->d_counts + RC_TAKEN,
                             e->stream, s.idx.a_lo, s.idx.a_off));
    TRY(next_scan(e, &sc));
    HIP_TRY(launch_take_keys(rows_of(rows_cat), r.ukeys, nu, rows_out_of(&s.ed), rows_cat->n, sc,
                             e->d_counts + RC_EDIT, e->stream, r.u_lo, r.e_off, r.u_len));
    HIP_TRY(launch_splice_index(sp, e->stream));
    TRY(read_counts(e));
    n_ak = e->h_counts[RC_TAKEN];
    n_e = e->h_counts[RC_EDIT];
    if (n_ak <= cap_k) break;
    if (attempt || n_ak > state->n) return fail(DG_E_DEVICE, "%s: the take counted %llu rows", WHAT, (unsigned long long)n_ak);
    cap_k = n_ak;
  }
  const bool moved = (u32)e->h_counts[RC_MOVED] != 0;
  dg_store ak = s.ak, ed = s.ed;
  ak.n = n_ak;
  ed.n = n_e;
  // 4. the tree first, with the taken rows as old and E as new: an input error (a key outside
  // the shard, a bucket over 65535 rows) is undone there and returned before a row is written
  if (tree) TRY(tree_update(e, tree, &ak, &ed, r.ukeys, nu, WHAT));
  // 5. the copy: in place when no key's row count changes, else into `spare`
  dg_store* out = moved ? spare : state;
  sp.out = rows_out_of(out);
  HIP_TRY(launch_splice_copy(sp, !moved, e->stream));
  TRY(read_counts(e));
  out->n = state->n - n_ak + n_e;
  if (moved) {
    std::swap(*state, *spare);
    *swapped = 1;
  }
  *n_union = nu;
  return DG_OK;
}

}  // extern "C"
