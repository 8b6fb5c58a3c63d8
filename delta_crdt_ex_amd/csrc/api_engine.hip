// api_engine.hip — the engine of libdeltagpu's C-ABI (include/deltagpu.h): its lifecycle, the
// grow-on-demand scratch, the publish-and-wait of a synchronous call, argument checks and
// dg_last_error.  Errors follow the header's conventions; nothing falls back to a CPU path.
#include <mutex>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "dg_engine.h"

// The single-pass join kernel is persistent: its workgroups wait on each other, so two
// of its grids must never be in flight on one device at once (each could hold CUs the
// other's waiting workgroups need).  While a device has one engine, its joins run on
// the engine's stream.  With several, every engine's join kernels run on one shared
// stream per device, ordered with the engine's own stream by events
// (tests/test_gpu_concurrency.py).  Against other streams' and processes' kernels the
// grid checks its own residency and aborts (join_stream.hip, stripe_sums); the calls then re-run
// on kernels that do not wait (dg_join2, dg_engine_sync, dg_join2_changes).
struct DevShare {
  int engines = 0;
  hipStream_t stream = nullptr;
};
std::mutex g_share_mu;
DevShare g_share[64];

// The device's shared join stream, or nullptr while e is the only engine on its device.
hipStream_t shared_join_stream(dg_engine* e) {
  std::lock_guard<std::mutex> g(g_share_mu);
  DevShare& d = g_share[e->device & 63];
  if (d.engines < 2) return nullptr;
  if (!d.stream && hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess)
    d.stream = nullptr;
  return d.stream;
}

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int set_device(dg_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  return DG_OK;
}

static_assert(sizeof(size_t) == sizeof(unsigned long long), "grow's messages take the count as %zu or %llu");

int grow(dg_engine* e, Buf* b, size_t need, size_t elem, size_t min_cap, int flags, const char* msg) {
  if (need <= b->cap) return DG_OK;
  const bool pinned = flags & GROW_PINNED;
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (b->p) HIP_TRY(pinned ? hipHostFree(b->p) : hipFree(b->p));
  b->p = nullptr;
  b->cap = 0;
  const size_t cap = std::max(need, min_cap);
  if ((pinned ? hipHostMalloc(&b->p, cap * elem, 0) : hipMalloc(&b->p, cap * elem)) != hipSuccess) {
    b->p = nullptr;
    return fail(DG_E_NOMEM, msg, (unsigned long long)cap);
  }
  // zeroed ON the engine stream, never by a plain hipMemset (see ensure_state)
  if (flags & GROW_ZERO) HIP_TRY(hipMemsetAsync(b->p, 0, cap * elem, e->stream));
  b->cap = cap;
  return DG_OK;
}

// A fresh epoch per look-back launch; granules of older epochs read as "not ready".
int next_scan(dg_engine* e, Scan* s) {
  if (++e->epoch >= (1u << 20)) {
    HIP_TRY(hipMemsetAsync(e->state.p, 0, e->state.cap * sizeof(u64), e->stream));
    if (e->counts.p) HIP_TRY(hipMemsetAsync(e->counts.p, 0, e->counts.cap * sizeof(u32), e->stream));
    HIP_TRY(hipMemsetAsync(e->started, 0, JOIN_MAX_GRID * sizeof(u32), e->stream));
    e->epoch = 1;
  }
  s->counts = e->counts.as<u32>();
  s->state = e->state.as<u64>();
  s->ticket = e->ticket + TK_TILE;
  s->err = e->ticket + TK_ERR;
  s->started = e->started;
  s->abort = e->ticket + TK_ABORT;
  s->epoch = e->epoch;
  return DG_OK;
}

namespace {

// Copies the engine's counts and error words into mapped host memory, then publishes the
// call's sequence number (system scope, after a system fence): when the host sees the
// number, everything before this kernel on the stream has finished and the copies landed.
__global__ void publish_counts_kernel(const u64* d, u64* h, u64 seq) {
  const int l = threadIdx.x;
  if (l < 16) h[l] = d[l];  // d_counts[0..8) and ticket[0..16)
  __threadfence_system();
  __syncthreads();
  if (l == 0) __hip_atomic_store(h + 16, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// The counts and the error bits (ticket[TK_ERR]) of a synchronous call: d_counts[0..8)
// and ticket[0..2) are contiguous on the device and land in h_counts[0..9).  Instead of a
// D2H copy and a stream synchronize (≈ 14 µs on top of a config-2 join), a one-wave kernel
// publishes them into mapped host memory and the host polls its sequence word; past 20 ms
// (a long call) the runtime's synchronize takes over, and it is what reports a fault.
// wait_published: the host side alone, for a launch that publishes `seq` itself (the
// small join's tail kernel).
int wait_published(dg_engine* e, u64 seq) {
  const volatile u64* flag = e->h_pub + 16;
  const auto t0 = std::chrono::steady_clock::now();
  bool seen = false;
  for (u32 i = 0;; i++) {
    if (*flag == seq) {
      seen = true;
      break;
    }
    if ((i & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    __builtin_ia32_pause();
  }
  if (!seen) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (*flag != seq) return fail(DG_E_DEVICE, "counts were not published");
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  memcpy(e->h_counts, (const void*)e->h_pub, 8 * sizeof(u64) + 2 * sizeof(u32));
  memcpy(e->h_ticket, (const void*)(e->h_pub + 8), sizeof(e->h_ticket));
  return DG_OK;
}

int sync_words(dg_engine* e) {
  const u64 seq = ++e->pub_seq;
  hipLaunchKernelGGL(publish_counts_kernel, dim3(1), dim3(WAVE), 0, e->stream, e->d_counts, e->d_pub, seq);
  HIP_TRY(hipGetLastError());
  return wait_published(e, seq);
}

int read_counts(dg_engine* e) {
  const int rc = sync_words(e);
  if (rc != DG_OK) return rc;
  return published_errors(e);
}

// the error bits of the count block just published (a look-back timeout, an aborted grid)
int published_errors(dg_engine* e) {
  e->last_err_bits = 0;
  u32 err = 0;
  memcpy(&err, (const char*)&e->h_counts[8] + TK_ERR * sizeof(u32), sizeof(u32));
  if (err) {
    e->last_err_bits = err;
    HIP_TRY(hipMemsetAsync(e->ticket, 0, 4 * sizeof(u32), e->stream));  // TK_TILE .. TK_INPUT
    static_assert(TAIL_ARRIVE == MERKLE_ARRIVE + 1, "the two arrival counters are cleared as one range");
    HIP_TRY(hipMemsetAsync(e->ticket + MERKLE_ARRIVE, 0, (TAIL_ARRIVE - MERKLE_ARRIVE + 1) * sizeof(u32), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return fail(DG_E_DEVICE, "a kernel timed out or a join grid aborted (error bits 0x%x)", err);
  }
  return DG_OK;
}

Rows rows_of(const dg_store* s) {
  Rows r;
  r.key = s->key;
  r.val = s->val;
  r.ts = s->ts;
  r.node = s->node;
  r.cnt = s->cnt;
  r.n = s->n;
  return r;
}

RowsOut rows_out_of(dg_store* s) {
  RowsOut r;
  r.key = s->key;
  r.val = s->val;
  r.ts = s->ts;
  r.node = s->node;
  r.cnt = s->cnt;
  return r;
}

Ctx ctx_of(const dg_context* c) {
  Ctx x;
  x.node = c->node;
  x.cnt = c->cnt;
  x.n = c->n;
  x.kind = c->kind;
  return x;
}

int copy_rows(dg_engine* e, const dg_store* dst, const dg_store* src, u64 n, hipMemcpyKind kind) {
  HIP_TRY(hipMemcpyAsync(dst->key, src->key, n * 8, kind, e->stream));
  HIP_TRY(hipMemcpyAsync(dst->val, src->val, n * 8, kind, e->stream));
  HIP_TRY(hipMemcpyAsync(dst->ts, src->ts, n * 8, kind, e->stream));
  HIP_TRY(hipMemcpyAsync(dst->node, src->node, n * 4, kind, e->stream));
  HIP_TRY(hipMemcpyAsync(dst->cnt, src->cnt, n * 8, kind, e->stream));
  return DG_OK;
}

int check_store(const dg_store* s, const char* what) {
  if (!s) return fail(DG_E_INVAL, "%s: null store", what);
  if (s->n && (!s->key || !s->val || !s->ts || !s->node || !s->cnt))
    return fail(DG_E_INVAL, "%s: null column with n=%llu", what, (unsigned long long)s->n);
  return DG_OK;
}

int check_ctx(const dg_context* c, const char* what) {
  if (!c) return fail(DG_E_INVAL, "%s: null context", what);
  if (c->kind != DG_CTX_VV && c->kind != DG_CTX_DOTS)
    return fail(DG_E_INVAL, "%s: bad context kind %d", what, c->kind);
  if (c->n && (!c->node || !c->cnt)) return fail(DG_E_INVAL, "%s: null context column", what);
  return DG_OK;
}

bool pair_aligned(const void* k, const void* v, const void* t, const void* n, const void* c) {
  return !(((uintptr_t)k | (uintptr_t)v | (uintptr_t)t | (uintptr_t)c) & 15) && !((uintptr_t)n & 7);
}

// Every synchronous entry point settles the asynchronous calls before it enqueues its own
// work: an aborted grid's error bit is then seen (and its calls replayed) by
// dg_engine_sync, never by the synchronous call's own error check, which would clear
// it and leave the aborted join's output unreported.
int settle(dg_engine* e) {
  if (!e->pending.empty()) return dg_engine_sync(e);
  return DG_OK;
}

MerkleT merkle_of(const dg_merkle* t) {
  MerkleT m;
  m.depth = t->depth;
  m.sb = t->shard_bits;
  m.shard = t->shard;
  m.nodes = t->nodes;
  m.counts = t->counts;
  m.th = TermH{};
  if (t->terms) {
    m.th.nh = t->terms->node_hash;
    m.th.nn = t->terms->node_hash ? t->terms->n_nodes : 0;
    m.th.vid = t->terms->val_id;
    m.th.vh = t->terms->val_hash;
    m.th.nv = (t->terms->val_id && t->terms->val_hash) ? t->terms->n_vals : 0;
    m.th.on = 1;
  }
  m.starts = t->starts;
  return m;
}

int check_merkle(const dg_merkle* t, const char* what) {
  if (!t || !t->nodes) return fail(DG_E_INVAL, "%s: null tree", what);
  if (!t->counts || ((uintptr_t)t->counts & 15))
    return fail(DG_E_INVAL, "%s: the tree's counts must be a 16-byte aligned device array", what);
  if (t->depth < 1 || t->depth > 28) return fail(DG_E_INVAL, "%s: depth %u not in 1..28", what, t->depth);
  if (t->shard_bits > 16 || t->depth + t->shard_bits > 44)
    return fail(DG_E_INVAL, "%s: shard_bits %u (depth %u)", what, t->shard_bits, t->depth);
  if (t->shard_bits ? (t->shard >> t->shard_bits) != 0 : t->shard != 0)
    return fail(DG_E_INVAL, "%s: shard %llu >= 2^%u", what, (unsigned long long)t->shard, t->shard_bits);
  return DG_OK;
}

int tree_input_error(u32 bits, const char* what, const char* holds) {
  if (bits & MERKLE_ERR_SHARD) return fail(DG_E_INVAL, "%s: a key outside the tree's shard", what);
  if (bits & MERKLE_ERR_COUNT)
    return fail(DG_E_CAPACITY, "%s: a bucket %s more than 65535 rows (use a deeper tree)", what, holds);
  return DG_OK;
}

extern "C" {

int dg_abi_version(void) { return DG_ABI_VERSION; }

const char* dg_last_error(void) { return g_err.c_str(); }

int dg_engine_create(int device, void* hip_stream, dg_engine** out) {
  if (!out) return fail(DG_E_INVAL, "dg_engine_create: null out");
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return fail(DG_E_INVAL, "dg_engine_create: device %d of %d", device, ndev);
  dg_engine* e = new dg_engine();
  e->device = device;
  {
    const char* v = getenv("DG_JOIN_WORKERS");
    if (v && atoi(v) > 0) e->join_workers = atoi(v);
    const char* sg = getenv("DG_JOIN_STAGGER");
    if (sg && atoi(sg) > 0) e->join_stagger = atoi(sg) < 4096 ? atoi(sg) : 4096;
    const char* m = getenv("DG_JOIN_MODE");
    if (m && m[0] == '2') e->join_mode = JOIN_TWO_PASS;
    const char* sp = getenv("DG_SPLICE");
    if (sp && sp[0] == '0') e->splice = false;
    const char* kd = getenv("DG_KD");
    if (kd && kd[0] == '0') e->kd = false;
    const char* am = getenv("DG_APPLY_MODE");
    if (am && strcmp(am, "fold") == 0) e->apply_mode = 1;
    if (am && strcmp(am, "onepass") == 0) e->apply_mode = 2;
    const char* tr = getenv("DG_TREE_REBUILD");
    if (tr && strcmp(tr, "always") == 0) e->tree_rebuild = dg_engine::TREE_ALWAYS;
    if (tr && strcmp(tr, "never") == 0) e->tree_rebuild = dg_engine::TREE_NEVER;
    if (tr && atoll(tr) > 0) e->tree_rebuild_div = (u64)atoll(tr);
  }
  int rc = set_device(e);
  if (rc != DG_OK) {
    delete e;
    return rc;
  }
  if (hip_stream) {
    e->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
      delete e;
      return fail(DG_E_DEVICE, "hipStreamCreate failed");
    }
    e->own_stream = true;
  }
  if (hipMalloc(&e->d_counts, 8 * sizeof(u64) + 16 * sizeof(u32)) != hipSuccess ||
      hipMalloc(&e->started, JOIN_MAX_GRID * sizeof(u32)) != hipSuccess ||
      hipHostMalloc(&e->h_counts, 16 * sizeof(u64), 0) != hipSuccess ||
      hipHostMalloc(&e->h_pub, 24 * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer((void**)&e->d_pub, e->h_pub, 0) != hipSuccess) {
    dg_engine_destroy(e);
    return fail(DG_E_NOMEM, "dg_engine_create: allocation failed");
  }
  e->ticket = (u32*)(e->d_counts + 8);
  memset(e->h_pub, 0, 24 * sizeof(u64));  // sequence 0: nothing published yet
  if (hipMemsetAsync(e->d_counts, 0, 8 * sizeof(u64) + 16 * sizeof(u32), e->stream) != hipSuccess ||
      hipMemsetAsync(e->started, 0, JOIN_MAX_GRID * sizeof(u32), e->stream) != hipSuccess) {
    dg_engine_destroy(e);
    return fail(DG_E_DEVICE, "dg_engine_create: hipMemsetAsync failed");
  }
  rc = ensure_state(e, 4096);
  if (rc != DG_OK) {
    dg_engine_destroy(e);
    return rc;
  }
  if (hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming) != hipSuccess) {
    dg_engine_destroy(e);
    return fail(DG_E_DEVICE, "dg_engine_create: hipEventCreate failed");
  }
  {
    std::lock_guard<std::mutex> g(g_share_mu);
    const int n = ++g_share[device & 63].engines;
    // the first engine's joins ran on its own stream: let them finish before any join of
    // this one can start, from here on they share a stream
    if (n == 2) hipDeviceSynchronize();
  }
  *out = e;
  return DG_OK;
}

int dg_engine_destroy(dg_engine* e) {
  if (!e) return DG_OK;
  hipSetDevice(e->device);
  if (e->stream) hipStreamSynchronize(e->stream);
  for (Buf* b : {&e->state, &e->tmp, &e->counts, &e->fold, &e->spl, &e->ubuf, &e->sml, &e->kdb, &e->kdz, &e->rpl,
                 &e->diff_bsum, &e->diff_rsum})
    if (b->p) hipFree(b->p);
  if (e->d_counts) hipFree(e->d_counts);
  if (e->h_counts) hipHostFree(e->h_counts);
  if (e->h_pub) hipHostFree(e->h_pub);
  if (e->started) hipFree(e->started);
  if (e->h_stage.p) hipHostFree(e->h_stage.p);
  if (e->h_cont.p) hipHostFree(e->h_cont.p);
  if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
  if (e->ev_in || e->ev_out) {  // a registered engine (creation got past the registry)
    if (e->ev_in) hipEventDestroy(e->ev_in);
    if (e->ev_out) hipEventDestroy(e->ev_out);
    std::lock_guard<std::mutex> g(g_share_mu);
    DevShare& d = g_share[e->device & 63];
    if (e->ev_out && --d.engines == 0 && d.stream) {
      hipStreamSynchronize(d.stream);
      hipStreamDestroy(d.stream);
      d.stream = nullptr;
    }
  }
  delete e;
  return DG_OK;
}

void* dg_engine_stream(dg_engine* e) { return e ? (void*)e->stream : nullptr; }

// Error bits of the work on the engine stream so far (synchronizes), cleared.
static int stream_error(dg_engine* e, u32* err) {
  TRY(sync_words(e));
  *err = e->h_ticket[TK_ERR];
  if (*err) {
    HIP_TRY(hipMemsetAsync(e->ticket, 0, 4 * sizeof(u32), e->stream));  // TK_TILE .. TK_INPUT
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return DG_OK;
}

int dg_engine_sync(dg_engine* e) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(set_device(e));
  u32 err = 0;
  TRY(stream_error(e, &err));
  if (err & 3u) {
    // a single-pass join grid aborted (not co-resident) or timed out: replay the
    // asynchronous calls since the last sync in order, the joins on the two-pass kernels
    // (their workgroups never wait on each other)
    std::vector<dg_engine::Pending> log;
    log.swap(e->pending);
    for (dg_engine::Pending& q : log) {
      if (q.kind == 0)
        TRY(join2_enqueue(e, &q.a, &q.ca, &q.b, &q.cb, q.keys, q.n_keys, &q.out, &q.out_ctx,
                          q.d_counts, nullptr, true));
      else
        TRY(merkle_build_enqueue(e, &q.a, q.tp, q.d_counts));
    }
    e->pending.clear();
    TRY(stream_error(e, &err));
  }
  e->pending.clear();
  if (err) return fail(DG_E_DEVICE, "kernel error bits 0x%x after dg_engine_sync", err);
  return DG_OK;
}

int dg_store_check(dg_engine* e, const dg_store* s) {
  if (!e) return fail(DG_E_INVAL, "null engine");
  TRY(check_store(s, "dg_store_check"));
  TRY(set_device(e));
  TRY(settle(e));
  HIP_TRY(hipMemsetAsync(e->ticket + TK_ORDER, 0, sizeof(u32), e->stream));
  HIP_TRY(launch_store_check(rows_of(s), e->ticket + TK_ORDER, e->stream));
  TRY(sync_words(e));
  if (e->h_ticket[TK_ORDER]) return fail(DG_E_ORDER, "store rows are not strictly ascending");
  return DG_OK;
}

}  // extern "C"
