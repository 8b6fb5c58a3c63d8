// api_merkle.hip — the Merkle calls of the C-ABI: build, update, diff and the
// continuation protocol.
#include "dg_engine.h"

namespace {

// one full diff enqueued: the group sums of this call and the ones its write kernel zeroes
// (all g words: a call of another depth may have dirtied more groups than this one has)
hipError_t enqueue_merkle_diff(dg_engine* e, const dg_merkle* a, const dg_store* sa, const dg_merkle* b,
                               const dg_store* sb, uint64_t* out_keys, uint64_t cap, u64* d_total) {
  const u64 g = e->diff_bsum.cap;
  u64* use = e->diff_bsum.as<u64>() + (e->diff_parity ? g : 0);
  u64* zero = e->diff_bsum.as<u64>() + (e->diff_parity ? 0 : g);
  e->diff_parity ^= 1;
  return launch_merkle_diff(merkle_of(a), rows_of(sa), merkle_of(b), rows_of(sb), out_keys, cap,
                            e->tmp.as<u64>(), use, zero, g, d_total, e->stream);
}

int same_tree_shape(const dg_merkle* a, const dg_merkle* b, const char* what) {
  if (a->depth != b->depth || a->shard_bits != b->shard_bits || a->shard != b->shard)
    return fail(DG_E_INVAL, "%s: trees of different shape (depth %u/%u, shard %llu/%llu)", what,
                a->depth, b->depth, (unsigned long long)a->shard, (unsigned long long)b->shard);
  return DG_OK;
}

}  // namespace

// The build's launch, shared by the synchronous call, the asynchronous one and the replay.
int merkle_build_enqueue(dg_engine* e, const dg_store* s, dg_merkle* t, uint64_t* d_n_keys) {
  TRY(check_store(s, "dg_merkle_build"));
  TRY(check_merkle(t, "dg_merkle_build"));
  if (!d_n_keys) return fail(DG_E_INVAL, "dg_merkle_build: null d_n_keys");
  TRY(set_device(e));
  TRY(ensure_tmp(e, merkle_ctr_words(t->depth) * sizeof(u32)));
  HIP_TRY(hipMemsetAsync(e->ticket + TK_INPUT, 0, sizeof(u32), e->stream));
  HIP_TRY(launch_merkle_build(rows_of(s), merkle_of(t), d_n_keys, e->ticket + MERKLE_ARRIVE,
                              e->tmp.as<u64>(), e->ticket + TK_INPUT, e->stream));
  return DG_OK;
}

extern "C" {

int dg_merkle_build_async(dg_engine* e, const dg_store* s, dg_merkle* t, uint64_t* d_n_keys) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  if (e->pending.size() >= MAX_PENDING) TRY(dg_engine_sync(e));
  TRY(merkle_build_enqueue(e, s, t, d_n_keys));
  dg_engine::Pending q{};
  q.kind = 1;
  q.a = *s;
  q.t = *t;
  q.tp = t;
  q.d_counts = d_n_keys;
  e->pending.push_back(q);
  return DG_OK;
}

int dg_merkle_build(dg_engine* e, const dg_store* s, dg_merkle* t) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(settle(e));
  TRY(merkle_build_enqueue(e, s, t, e->d_counts));  // not logged: it is settled right here
  TRY(read_counts(e));
  TRY(tree_input_error(e->h_ticket[TK_INPUT], "dg_merkle_build"));
  t->n_keys = e->h_counts[JC_ROWS];
  return DG_OK;
}

int dg_merkle_update(dg_engine* e, dg_merkle* t, const dg_store* old_s, const dg_store* new_s,
                     const uint64_t* keys, uint64_t n_keys) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(t, "dg_merkle_update"));
  TRY(check_store(old_s, "dg_merkle_update old"));
  TRY(check_store(new_s, "dg_merkle_update new"));
  if (n_keys && !keys) return fail(DG_E_INVAL, "dg_merkle_update: null keys");
  TRY(set_device(e));
  TRY(settle(e));
  return tree_update(e, t, old_s, new_s, keys, n_keys, "dg_merkle_update");
}

int dg_merkle_diff(dg_engine* e, const dg_merkle* a, const dg_store* sa, const dg_merkle* b,
                   const dg_store* sb, uint64_t* out_keys, uint64_t cap, uint64_t* n_out,
                   uint64_t* n_total) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(a, "dg_merkle_diff a"));
  TRY(check_merkle(b, "dg_merkle_diff b"));
  TRY(same_tree_shape(a, b, "dg_merkle_diff"));
  TRY(check_store(sa, "dg_merkle_diff sa"));
  TRY(check_store(sb, "dg_merkle_diff sb"));
  if (!n_out) return fail(DG_E_INVAL, "dg_merkle_diff: null n_out");
  if (cap && !out_keys) return fail(DG_E_INVAL, "dg_merkle_diff: null out_keys");
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_tmp(e, diff_scratch_words(a->depth, sa->n, sb->n) * sizeof(u64)));
  TRY(ensure_diff_bsum(e, diff_groups(a->depth)));
  HIP_TRY(enqueue_merkle_diff(e, a, sa, b, sb, out_keys, cap, e->d_counts));
  TRY(read_counts(e));
  const u64 total = e->h_counts[JC_ROWS];
  if (total >= DIFF_MISMATCH) {
    *n_out = 0;
    if (n_total) *n_total = 0;
    return fail(DG_E_INVAL, "dg_merkle_diff: a tree counts more rows than its store holds "
                            "(the store is not the one the tree was built / updated against)");
  }
  *n_out = std::min<u64>(total, cap);
  if (n_total) *n_total = total;
  return DG_OK;
}

int dg_merkle_diff_take(dg_engine* e, const dg_merkle* a, const dg_store* sa, const dg_merkle* b,
                        const dg_store* sb, int side, uint64_t* out_keys, uint64_t cap, uint64_t* offs,
                        dg_store* rows, uint64_t* n_out, uint64_t* n_total) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(a, "dg_merkle_diff_take a"));
  TRY(check_merkle(b, "dg_merkle_diff_take b"));
  TRY(same_tree_shape(a, b, "dg_merkle_diff_take"));
  TRY(check_store(sa, "dg_merkle_diff_take sa"));
  TRY(check_store(sb, "dg_merkle_diff_take sb"));
  if (side != 0 && side != 1) return fail(DG_E_INVAL, "dg_merkle_diff_take: side %d (0: sa, 1: sb)", side);
  if (!n_out) return fail(DG_E_INVAL, "dg_merkle_diff_take: null n_out");
  if (cap && !out_keys) return fail(DG_E_INVAL, "dg_merkle_diff_take: null out_keys");
  if (cap && !offs) return fail(DG_E_INVAL, "dg_merkle_diff_take: null offs");
  if (!rows) return fail(DG_E_INVAL, "dg_merkle_diff_take: null rows");
  if (rows->cap && (!rows->key || !rows->val || !rows->ts || !rows->node || !rows->cnt))
    return fail(DG_E_INVAL, "dg_merkle_diff_take: null column with cap=%llu", (unsigned long long)rows->cap);
  TRY(set_device(e));
  TRY(settle(e));
  rows->n = 0;
  TRY(ensure_tmp(e, diff_take_scratch_words(a->depth, sa->n, sb->n) * sizeof(u64)));
  TRY(ensure_diff_bsum(e, diff_groups(a->depth)));
  TRY(ensure_diff_rsum(e, diff_groups(a->depth)));
  {
    const u64 g = e->diff_bsum.cap, rg = e->diff_rsum.cap;
    u64* use = e->diff_bsum.as<u64>() + (e->diff_parity ? g : 0);
    u64* zero = e->diff_bsum.as<u64>() + (e->diff_parity ? 0 : g);
    u64* ruse = e->diff_rsum.as<u64>() + (e->diff_rparity ? rg : 0);
    u64* rzero = e->diff_rsum.as<u64>() + (e->diff_rparity ? 0 : rg);
    e->diff_parity ^= 1;
    e->diff_rparity ^= 1;
    HIP_TRY(launch_merkle_diff_take(merkle_of(a), rows_of(sa), merkle_of(b), rows_of(sb), (u32)side, out_keys, cap,
                                    offs, rows_out_of(rows), rows->cap, e->tmp.as<u64>(), use, zero, ruse, rzero, g,
                                    rg, e->d_counts, e->stream));
  }
  TRY(read_counts(e));  // the key total and the kept keys' rows, one wait
  const u64 total = e->h_counts[JC_ROWS];
  if (total >= DIFF_MISMATCH) {
    *n_out = 0;
    if (n_total) *n_total = 0;
    return fail(DG_E_INVAL, "dg_merkle_diff_take: a tree counts more rows than its store holds "
                            "(the store is not the one the tree was built / updated against)");
  }
  *n_out = std::min<u64>(total, cap);
  if (n_total) *n_total = total;
  rows->n = e->h_counts[DT_ROWS];
  if (rows->n > rows->cap)
    return fail(DG_E_CAPACITY, "dg_merkle_diff_take: %llu rows needed, room for %llu", (unsigned long long)rows->n,
                (unsigned long long)rows->cap);
  return DG_OK;
}

int dg_merkle_diff_async(dg_engine* e, const dg_merkle* a, const dg_store* sa, const dg_merkle* b,
                         const dg_store* sb, uint64_t* out_keys, uint64_t cap, uint64_t* d_total) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(a, "dg_merkle_diff_async a"));
  TRY(check_merkle(b, "dg_merkle_diff_async b"));
  TRY(same_tree_shape(a, b, "dg_merkle_diff_async"));
  TRY(check_store(sa, "dg_merkle_diff_async sa"));
  TRY(check_store(sb, "dg_merkle_diff_async sb"));
  if (!d_total) return fail(DG_E_INVAL, "dg_merkle_diff_async: null d_total");
  if (cap && !out_keys) return fail(DG_E_INVAL, "dg_merkle_diff_async: null out_keys");
  TRY(set_device(e));
  TRY(settle(e));  // (a logged join that aborted is replayed before its output is read)
  TRY(ensure_tmp(e, diff_scratch_words(a->depth, sa->n, sb->n) * sizeof(u64)));
  TRY(ensure_diff_bsum(e, diff_groups(a->depth)));
  HIP_TRY(enqueue_merkle_diff(e, a, sa, b, sb, out_keys, cap, d_total));
  return DG_OK;
}

int dg_merkle_prepare(dg_engine* e, const dg_merkle* t, uint32_t levels, dg_merkle_cont* out) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(t, "dg_merkle_prepare"));
  if (!out || levels < 1) return fail(DG_E_INVAL, "dg_merkle_prepare: bad arguments");
  const u32 L = std::min<u32>(levels, t->depth);
  const u64 n = 1ull << L;
  out->level = L;
  out->n = n;
  out->n_buckets = 0;
  if (out->cap < n || !out->pos || !out->hash)
    return fail(DG_E_CAPACITY, "dg_merkle_prepare: %llu entries needed", (unsigned long long)n);
  TRY(set_device(e));
  TRY(settle(e));
  HIP_TRY(launch_cont_prepare(merkle_of(t), L, out->pos, out->hash, e->stream));
  return sync_words(e);
}

int dg_merkle_continue(dg_engine* e, const dg_merkle* t, const dg_store* s, const dg_merkle_cont* in,
                       uint32_t levels, dg_merkle_cont* out, uint64_t* keys, uint64_t cap,
                       uint64_t* n_keys, uint64_t* n_total, int* status) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(t, "dg_merkle_continue"));
  TRY(check_store(s, "dg_merkle_continue"));
  if (!in || !status || !n_keys || levels < 1 || (cap && !keys))
    return fail(DG_E_INVAL, "dg_merkle_continue: bad arguments");
  if (in->n && (!in->pos || !in->hash)) return fail(DG_E_INVAL, "dg_merkle_continue: null input");
  *n_keys = 0;
  if (n_total) *n_total = 0;
  *status = 0;
  TRY(set_device(e));
  TRY(settle(e));
  const u32 depth = t->depth;
  const MerkleT m = merkle_of(t);
  if (in->level == depth + 1) {  // leaf form: the keys
    if (in->n_buckets && !in->bucket) return fail(DG_E_INVAL, "dg_merkle_continue: null buckets");
    TRY(ensure_state(e, 2 * cont_tiles(in->n_buckets) + 2));
    HIP_TRY(launch_leafdiff(m, rows_of(s), in->bucket, in->n_buckets, in->pos, in->hash, in->n, keys,
                            cap, e->state.as<u64>(), e->d_counts, e->stream));
    TRY(read_counts(e));
    const u64 total = e->h_counts[JC_ROWS];
    *n_keys = std::min<u64>(total, cap);
    if (n_total) *n_total = total;
    return DG_OK;
  }
  if (in->level > depth) return fail(DG_E_INVAL, "dg_merkle_continue: level %u > depth %u", in->level, depth);
  if (!out) return fail(DG_E_INVAL, "dg_merkle_continue: null out");
  const u32 L = in->level;
  TRY(ensure_state(e, 2 * cont_tiles(in->n) + 2));
  TRY(ensure_tmp(e, std::max<u64>(in->n, 1) * sizeof(u64)));
  u64* dpos = e->tmp.as<u64>();
  HIP_TRY(launch_cont_compare(m, L, in->pos, in->hash, in->n, e->state.as<u64>(), dpos, e->d_counts, e->stream));
  TRY(read_counts(e));
  const u64 nd = e->h_counts[JC_ROWS];
  if (nd == 0) return DG_OK;  // {:ok, []}
  if (L < depth) {
    const u32 k = std::min<u32>(levels, depth - L);
    const u64 need = nd << k;
    out->level = L + k;
    out->n = need;
    out->n_buckets = 0;
    if (out->cap < need || !out->pos || !out->hash)
      return fail(DG_E_CAPACITY, "dg_merkle_continue: %llu entries needed", (unsigned long long)need);
    HIP_TRY(launch_cont_expand(m, L, k, dpos, nd, out->pos, out->hash, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *status = 1;
    return DG_OK;
  }
  // the differing buckets -> leaf form
  out->level = depth + 1;
  out->n_buckets = nd;
  if (out->cap_buckets < nd || !out->bucket)
    return fail(DG_E_CAPACITY, "dg_merkle_continue: %llu buckets needed", (unsigned long long)nd);
  HIP_TRY(hipMemcpyAsync(out->bucket, dpos, nd * sizeof(u64), hipMemcpyDeviceToDevice, e->stream));
  TRY(ensure_state(e, 2 * cont_tiles(nd) + 2));
  HIP_TRY(launch_leaves_count(m, rows_of(s), out->bucket, nd, e->state.as<u64>(), e->d_counts, e->stream));
  TRY(read_counts(e));
  const u64 np = e->h_counts[JC_ROWS];
  out->n = np;
  if (out->cap < np || (np && (!out->pos || !out->hash)))
    return fail(DG_E_CAPACITY, "dg_merkle_continue: %llu leaf pairs needed", (unsigned long long)np);
  HIP_TRY(launch_leaves_write(m, rows_of(s), out->bucket, nd, e->state.as<u64>(), out->pos, out->hash, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *status = 1;
  return DG_OK;
}

int dg_merkle_continue_home(dg_engine* e, const dg_merkle* t, const dg_store* s, const dg_merkle_cont* in,
                            uint32_t levels, uint64_t max, dg_merkle_cont* out, uint64_t* keys, uint64_t cap,
                            uint64_t* n_keys, uint64_t* n_total, int* status) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(t, "dg_merkle_continue_home"));
  TRY(check_store(s, "dg_merkle_continue_home"));
  if (!in || !status || !n_keys || levels < 1 || (cap && !keys))
    return fail(DG_E_INVAL, "dg_merkle_continue_home: bad arguments");
  if (in->n && (!in->pos || !in->hash)) return fail(DG_E_INVAL, "dg_merkle_continue_home: null input");
  const u32 depth = t->depth;
  const bool leaf = in->level == depth + 1;
  if (in->level > depth + 1) return fail(DG_E_INVAL, "dg_merkle_continue_home: level %u > depth %u", in->level, depth);
  if (leaf && in->n_buckets && !in->bucket) return fail(DG_E_INVAL, "dg_merkle_continue_home: null buckets");
  *n_keys = 0;
  if (n_total) *n_total = 0;
  *status = DG_CONT_DECLINED;
  if (in->n > CS_IN || (leaf && in->n_buckets > CS_B)) return DG_OK;  // the general path
  *status = 0;
  if (leaf ? in->n_buckets == 0 : in->n == 0) return DG_OK;  // {:ok, []}
  if (!leaf && !out) return fail(DG_E_INVAL, "dg_merkle_continue_home: null out");
  TRY(set_device(e));
  TRY(settle(e));
  ContSmallArgs a{};
  a.t = merkle_of(t);
  a.s = rows_of(s);
  a.level = in->level;
  a.levels = levels;
  a.max = max;
  a.ipos = in->pos;
  a.ihash = in->hash;
  a.ibucket = leaf ? in->bucket : nullptr;
  a.n = in->n;
  a.nb = leaf ? in->n_buckets : 0;
  if (out) {
    a.opos = out->pos;
    a.ohash = out->hash;
    a.obucket = out->bucket;
    a.ocap = out->pos && out->hash ? out->cap : 0;
    a.ocap_b = out->bucket ? out->cap_buckets : 0;
  }
  a.keys = keys;
  a.kcap = cap;
  a.home = e->d_pub + CONT_HOME;
  a.d_counts = e->d_counts;
  a.h_pub = e->d_pub;
  a.seq = ++e->pub_seq;
  HIP_TRY(launch_cont_small(a, e->stream));
  TRY(wait_published(e, a.seq));
  u64 h[CS_HDR];
  memcpy(h, (const void*)(e->h_pub + CONT_HOME), sizeof h);
  if (h[0] == CS_BAD)
    return fail(DG_E_INVAL, "dg_merkle_continue_home: a position or bucket outside the tree");
  if (h[0] == CS_CAP) {
    out->level = (u32)h[3];
    out->n = h[4];
    out->n_buckets = h[5];
    *status = 0;
    return fail(DG_E_CAPACITY, "dg_merkle_continue_home: %llu entries / %llu buckets needed",
                (unsigned long long)h[4], (unsigned long long)h[5]);
  }
  if (h[0] == CS_OK) {
    *n_keys = std::min<u64>(h[1], cap);
    if (n_total) *n_total = h[1];
    return DG_OK;
  }
  out->level = (u32)h[3];
  out->n = h[1];
  out->n_buckets = h[0] == CS_LEAF ? h[2] : 0;
  *status = 1;
  return DG_OK;
}

static_assert(DG_CONT_BATCH_MAX == CONT_BATCH_MAX, "deltagpu.h's batch limit is the kernel's");
static_assert(sizeof(ContHop) % sizeof(u64) == 0 && sizeof(ContTakeHop) % sizeof(u64) == 0,
              "descriptors are whole words of the page-locked block");

}  // extern "C"

namespace {

// dg_merkle_continues (takes == nullptr) and dg_merkle_continues_take
int merkle_continues(dg_engine* e, const dg_merkle* t, const dg_store* s, int k, dg_cont_hop* hops,
                     dg_cont_take* const* takes, uint32_t levels, uint64_t max, const char* what) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_merkle(t, what));
  TRY(check_store(s, what));
  if (k < 0 || k > CONT_BATCH_MAX) return fail(DG_E_INVAL, "%s: k = %d hops (0 .. %d)", what, k, CONT_BATCH_MAX);
  if ((k > 0 && !hops) || levels < 1) return fail(DG_E_INVAL, "%s: bad arguments", what);
  if (k == 0) return DG_OK;
  for (int j = 0; takes && j < k; j++) {
    dg_cont_take* tk = takes[j];
    if (!tk) continue;
    if (!tk->offs) return fail(DG_E_INVAL, "%s: take %d: null offs", what, j);
    const dg_store& r = tk->rows;
    if (r.cap && (!r.key || !r.val || !r.ts || !r.node || !r.cnt))
      return fail(DG_E_INVAL, "%s: take %d: null column with cap=%llu", what, j, (unsigned long long)r.cap);
    if (!hops[j].keys || !hops[j].cap) return fail(DG_E_INVAL, "%s: take %d: its hop has no room for keys", what, j);
    tk->rows.n = 0;
    tk->rc = DG_OK;
  }
  // each hop's own checks, exactly dg_merkle_continue_home's
  const u32 depth = t->depth;
  std::vector<std::string> msgs(k);
  auto hop_fail = [&](int j, int code, const char* fmt, unsigned long long a, unsigned long long b) {
    char msg[256];
    snprintf(msg, sizeof msg, fmt, a, b);
    msgs[j] = msg;
    hops[j].rc = code;
  };
  int slot[CONT_BATCH_MAX];  // workgroup -> hop
  u32 nw = 0;
  for (int j = 0; j < k; j++) {
    dg_cont_hop& h = hops[j];
    const dg_merkle_cont* in = h.in;
    h.n_keys = h.n_total = 0;
    h.status = 0;
    h.rc = DG_OK;
    if (!in || (h.cap && !h.keys)) { hop_fail(j, DG_E_INVAL, "bad arguments", 0, 0); continue; }
    if (in->n && (!in->pos || !in->hash)) { hop_fail(j, DG_E_INVAL, "null input", 0, 0); continue; }
    const bool leaf = in->level == depth + 1;
    if (in->level > depth + 1) { hop_fail(j, DG_E_INVAL, "level %llu > depth %llu", in->level, depth); continue; }
    if (leaf && in->n_buckets && !in->bucket) { hop_fail(j, DG_E_INVAL, "null buckets", 0, 0); continue; }
    h.status = DG_CONT_DECLINED;
    if (in->n > CS_IN || (leaf && in->n_buckets > CS_B)) continue;  // the general path
    h.status = 0;
    if (leaf ? in->n_buckets == 0 : in->n == 0) continue;  // {:ok, []}
    if (!leaf && !h.out) { hop_fail(j, DG_E_INVAL, "null out", 0, 0); continue; }
    slot[nw++] = j;
  }
  if (nw) {
    TRY(set_device(e));
    TRY(settle(e));
    // rows can only come of a leaf form: a batch without one that asks for rows is the plain launch
    bool take = false;
    for (u32 w = 0; takes && w < nw; w++) take |= takes[slot[w]] && hops[slot[w]].in->level == depth + 1;
    const size_t desc_words = sizeof(ContHop) / sizeof(u64), take_words = sizeof(ContTakeHop) / sizeof(u64);
    TRY(ensure_cont(e, (size_t)CONT_BATCH_MAX * (desc_words + CONT_HDR_STRIDE + (take ? take_words : 0))));
    ContHop* hd = e->h_cont.as<ContHop>();
    u64* hdr = e->h_cont.as<u64>() + (size_t)CONT_BATCH_MAX * desc_words;
    ContTakeHop* td = (ContTakeHop*)(hdr + (size_t)CONT_BATCH_MAX * CONT_HDR_STRIDE);
    for (u32 w = 0; w < nw; w++) {
      const dg_cont_hop& h = hops[slot[w]];
      const dg_merkle_cont* in = h.in;
      const bool leaf = in->level == depth + 1;
      ContHop d{};
      d.level = in->level;
      d.n = in->n;
      d.nb = leaf ? in->n_buckets : 0;
      d.ipos = in->pos;
      d.ihash = in->hash;
      d.ibucket = leaf ? in->bucket : nullptr;
      if (h.out) {
        d.opos = h.out->pos;
        d.ohash = h.out->hash;
        d.obucket = h.out->bucket;
        d.ocap = h.out->pos && h.out->hash ? h.out->cap : 0;
        d.ocap_b = h.out->bucket ? h.out->cap_buckets : 0;
      }
      d.keys = h.keys;
      d.kcap = h.cap;
      hd[w] = d;
      if (take) {
        ContTakeHop x{};
        if (dg_cont_take* tk = leaf ? takes[slot[w]] : nullptr) {
          x.rows = rows_out_of(&tk->rows);
          x.rcap = tk->rows.cap;
          x.offs = tk->offs;
        }
        td[w] = x;
      }
    }
    ContTakeArgs p{};
    p.t = merkle_of(t);
    p.s = rows_of(s);
    p.levels = levels;
    p.max = max;
    p.hops = hd;
    p.hdr = hdr;
    p.arrive = e->ticket + CONT_ARRIVE;
    p.d_counts = e->d_counts;
    p.h_pub = e->d_pub;
    p.seq = ++e->pub_seq;
    p.takes = td;
    HIP_TRY(take ? launch_cont_take(p, nw, e->stream) : launch_cont_batch(p, nw, e->stream));
    TRY(wait_published(e, p.seq));
    for (u32 w = 0; w < nw; w++) {
      const int j = slot[w];
      dg_cont_hop& h = hops[j];
      u64 r[CS_HDR];
      memcpy(r, (const void*)(hdr + (size_t)w * CONT_HDR_STRIDE), sizeof r);
      if (r[0] == CS_BAD) {
        hop_fail(j, DG_E_INVAL, "a position or bucket outside the tree", 0, 0);
      } else if (r[0] == CS_CAP) {
        h.out->level = (u32)r[3];
        h.out->n = r[4];
        h.out->n_buckets = r[5];
        hop_fail(j, DG_E_CAPACITY, "%llu entries / %llu buckets needed", r[4], r[5]);
      } else if (r[0] == CS_OK) {
        h.n_keys = std::min<u64>(r[1], h.cap);
        h.n_total = r[1];
        if (take && td[w].offs) {  // (written by the workgroup with every CS_OK of a leaf form)
          dg_cont_take* tk = takes[j];
          memcpy(&tk->rows.n, (const void*)(hdr + (size_t)w * CONT_HDR_STRIDE + CS_TAKEN), sizeof(u64));
          if (tk->rows.n > tk->rows.cap) tk->rc = DG_E_CAPACITY;
        }
      } else {
        h.out->level = (u32)r[3];
        h.out->n = r[1];
        h.out->n_buckets = r[0] == CS_LEAF ? r[2] : 0;
        h.status = 1;
      }
    }
  }
  for (int j = 0; j < k; j++)
    if (hops[j].rc != DG_OK) {
      fail(hops[j].rc, "%s: hop %d: %s", what, j, msgs[j].c_str());
      break;
    }
  return DG_OK;
}

}  // namespace

extern "C" {

int dg_merkle_continues(dg_engine* e, const dg_merkle* t, const dg_store* s, int k, dg_cont_hop* hops,
                        uint32_t levels, uint64_t max) {
  return merkle_continues(e, t, s, k, hops, nullptr, levels, max, "dg_merkle_continues");
}

int dg_merkle_continues_take(dg_engine* e, const dg_merkle* t, const dg_store* s, int k, dg_cont_hop* hops,
                             dg_cont_take* const* takes, uint32_t levels, uint64_t max) {
  return merkle_continues(e, t, s, k, hops, takes, levels, max,
                          takes ? "dg_merkle_continues_take" : "dg_merkle_continues");
}

int dg_merkle_truncate(dg_engine* e, const dg_merkle* t, dg_merkle_cont* cont, uint64_t max) {
  if (!e || !cont) return fail(DG_E_INVAL, "dg_merkle_truncate: null argument");
  TRY(check_merkle(t, "dg_merkle_truncate"));
  if (cont->n_buckets == 0 || cont->bucket == nullptr) {  // node form (or an empty leaf form)
    cont->n = std::min<u64>(cont->n, max);
    return DG_OK;
  }
  if (cont->n_buckets <= max) return DG_OK;
  // leaf form: the pairs of the first `max` buckets are those whose key sorts before
  // the first pair of bucket[max]; pairs carry keys, buckets carry bucket numbers, so
  // count the pairs of the dropped buckets by their bucket's first pair
  TRY(set_device(e));
  TRY(settle(e));
  TRY(ensure_state(e, 2));
  HIP_TRY(launch_pairs_before_bucket(merkle_of(t), cont->pos, cont->n, cont->bucket + max,
                                     e->d_counts, e->stream));
  TRY(read_counts(e));
  cont->n = e->h_counts[JC_ROWS];
  cont->n_buckets = max;
  return DG_OK;
}

uint64_t dg_merkle_chunks(uint32_t depth) { return merkle_chunks(depth); }

int dg_merkle_fold_roots(const uint64_t* roots, uint32_t shard_bits, uint64_t* root) {
  if (!roots || !root || shard_bits > 16) return fail(DG_E_INVAL, "dg_merkle_fold_roots: bad arguments");
  std::vector<u64> lvl(roots, roots + (1ull << shard_bits));
  while (lvl.size() > 1) {
    std::vector<u64> up(lvl.size() / 2);
    for (size_t i = 0; i < up.size(); i++) up[i] = node_hash(lvl[2 * i], lvl[2 * i + 1]);
    lvl.swap(up);
  }
  *root = lvl[0];
  return DG_OK;
}

}  // extern "C"
