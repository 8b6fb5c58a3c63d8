// api_takesets.hip — dg_take_keysets: the values of k pending sync deltas out of one pass.
// The keysets' union with per-key set masks (takesets.hip), then ONE take of the union
// (take.hip), whose per-key offsets say which rows are which key's.
#include "dg_engine.h"

namespace {

enum TakesetsCount {  // e->d_counts of this path
  TS_ROWS = JC_ROWS,  // the union's rows (take_keys_kernel)
  TS_KEYS = 1,        // union keys (keysets_union_kernel)
};
constexpr size_t HIST8_BYTES = 8 * 256 * sizeof(u32);  // sort_fields' pinned byte counts

}  // namespace

extern "C" {

int dg_take_keysets(dg_engine* e, const dg_store* s, int k, const uint64_t* const* keys, const uint64_t* n_keys,
                    uint64_t* ukeys, uint64_t* masks, uint64_t* offs, uint64_t cap_keys, uint64_t* n_ukeys,
                    dg_store* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(s, "dg_take_keysets"));
  if (!n_ukeys) return fail(DG_E_INVAL, "dg_take_keysets: null n_ukeys");
  *n_ukeys = 0;
  if (!out || !offs) return fail(DG_E_INVAL, "dg_take_keysets: null argument");
  if (k < 0 || k > KS_MAX_K) return fail(DG_E_INVAL, "dg_take_keysets: k = %d keysets (0 .. %d)", k, KS_MAX_K);
  if (k > 0 && (!keys || !n_keys)) return fail(DG_E_INVAL, "dg_take_keysets: null keysets");
  if (cap_keys && (!ukeys || !masks)) return fail(DG_E_INVAL, "dg_take_keysets: null output array");
  if (out->cap && (!out->key || !out->val || !out->ts || !out->node || !out->cnt))
    return fail(DG_E_INVAL, "dg_take_keysets: null output column");
  u64 m = 0;
  for (int j = 0; j < k; j++) {
    if (n_keys[j] && !keys[j]) return fail(DG_E_INVAL, "dg_take_keysets: keys NULL with n_keys>0");
    if (n_keys[j] >= (1ull << 32)) return fail(DG_E_INVAL, "dg_take_keysets: a keyset of more than 2^32 - 1 keys");
    m += n_keys[j];
  }
  if (m >= (1ull << 32)) return fail(DG_E_INVAL, "dg_take_keysets: more than 2^32 - 1 keys in all");
  TRY(set_device(e));
  TRY(settle(e));
  if (m == 0) {  // no key: no row
    static const u64 zero = 0;
    HIP_TRY(hipMemcpyAsync(offs, &zero, sizeof zero, hipMemcpyDefault, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    out->n = 0;
    return DG_OK;
  }
  // every buffer grown before any pointer into one is taken
  TRY(ensure_stage(e, HIST8_BYTES + (size_t)(k + 1) * sizeof(KsSeg)));
  TRY(ensure_state(e, std::max(ks_tiles(m), take_tiles(m)) + 1));
  TakesetsScratch t;
  TRY(carve(e, &e->tmp, [&](Arena& a) { return takesets_layout(a, (u64)k, sizeof(KsSeg), m, sort_tmp_bytes(m)); }, &t));
  u32* h_hist8 = e->h_stage.as<u32>();
  KsSeg* hs = (KsSeg*)(e->h_stage.as<char>() + HIST8_BYTES);
  u64 off = 0;
  for (int j = 0; j < k; j++) {
    hs[j] = KsSeg{keys[j], off};
    off += n_keys[j];
  }
  hs[k] = KsSeg{nullptr, m};
  KsSeg* ds = (KsSeg*)t.segs;
  HIP_TRY(hipMemcpyAsync(ds, hs, (size_t)(k + 1) * sizeof(KsSeg), hipMemcpyHostToDevice, e->stream));
  u32* bad = e->ticket + TK_INPUT;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(u32), e->stream));
  HIP_TRY(launch_keysets_gather(ds, k, m, t.cat, t.set, bad, e->stream));
  // (the order flag before the sort: the union kernel's runs are at most k items long only
  // when every keyset is unique)
  TRY(read_counts(e));
  if (e->h_ticket[TK_INPUT]) return fail(DG_E_ORDER, "dg_take_keysets: a keyset is not strictly ascending");
  const SortField f{t.cat, 8, 0};
  u32* idx = nullptr;
  HIP_TRY(sort_fields(&f, 1, m, t.sort_tmp, &idx, h_hist8, e->stream));
  Scan sc;
  TRY(next_scan(e, &sc));
  HIP_TRY(launch_keysets_union(t.cat, t.set, idx, m, t.ukeys, ukeys, masks, cap_keys, sc, e->d_counts + TS_KEYS,
                               e->stream));
  TRY(read_counts(e));
  const u64 nu = e->h_counts[TS_KEYS];
  // the rows: the take of the union, its per-key offsets kept (more rows than out->cap are
  // counted, not written)
  TRY(next_scan(e, &sc));
  HIP_TRY(launch_take_keys(rows_of(s), t.ukeys, nu, rows_out_of(out), out->cap, sc, e->d_counts + TS_ROWS,
                           e->stream, t.key_lo, t.key_off));
  if (nu <= cap_keys)
    HIP_TRY(hipMemcpyAsync(offs, t.key_off, (nu + 1) * sizeof(u64), hipMemcpyDefault, e->stream));
  TRY(read_counts(e));
  *n_ukeys = nu;
  out->n = e->h_counts[TS_ROWS];
  if (nu > cap_keys || out->n > out->cap)
    return fail(DG_E_CAPACITY, "dg_take_keysets: needs %llu union keys (cap %llu), %llu rows (cap %llu)",
                (unsigned long long)nu, (unsigned long long)cap_keys, (unsigned long long)out->n,
                (unsigned long long)out->cap);
  return DG_OK;
}

}  // extern "C"
