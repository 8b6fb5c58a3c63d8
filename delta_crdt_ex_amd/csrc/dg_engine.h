// dg_engine.h — what the C-ABI layer's translation units (api_*.hip) share: the engine,
// the error helpers, the names of the engine's device words, and the helpers' prototypes.
// Internal: nothing here is part of include/deltagpu.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/deltagpu.h"
#include "dg_arena.h"
#include "dg_hash.h"
#include "dg_launch.h"

using namespace dg;

// Scratch that grows on demand (grow): cap counts elements of the size its owner grows it by.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T>
  T* as() const { return (T*)p; }
};

struct dg_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Buf state;              // decoupled look-back granules (u64)
  u32* ticket = nullptr;  // the Ticket words (16, right behind d_counts: one allocation, see below)
  Buf counts;             // single-pass join tile-count granules (u32)
  u32* started = nullptr;  // single-pass join start flags (JOIN_MAX_GRID epochs)
  Buf fold;               // ping-pong intermediate states of dg_joink / dg_apply_deltas
  bool splice = true;     // sparse keyed joins as a splice (DG_SPLICE=0: the full join)
  // the splice's taken rows, edit and per-key index (its own: a stepwise fold's joins
  // splice while their inputs live in `fold`)
  Buf spl;
  // dg_join_delta's union context on its full-join path (its own: the join it calls may
  // splice through `spl`)
  Buf ubuf;
  Buf sml;  // dg_join_delta_home's scratch: the edit, the per-key index, the result header
  // dg_join_delta's one-wait path (kdelta.hip): per-key figures, the splice index, the
  // union context (DG_KD=0: the splice path with its host waits, for A/B)
  Buf kdb;
  Buf rpl;  // dg_replace_keysets' per-item and per-union-key arrays (its own: the tree update
            //   behind them carves `tmp`, the splice `spl`)
  Buf kdz;  // its tree update's dirty flags and chunk row-count changes: zero between calls
            //   (the re-reduction consumes them)
  bool kd = true;
  // the full diff's per-group key sums: two buffers of diff_bsum.cap words, zero when
  // allocated; a call adds into one and its write kernel zeroes the other, which the
  // previous call used (no memset launch per diff)
  Buf diff_bsum;
  int diff_parity = 0;
  // dg_merkle_diff_take's per-group row sums, kept the same way with a parity of their own:
  // only a take adds into them, and only a take's write kernel zeroes the previous take's
  Buf diff_rsum;
  int diff_rparity = 0;
  u32 epoch = 0;
  // small device counters + pinned host mirror.  d_counts[0..8) and ticket[0..16) are one
  // device allocation (ticket == (u32*)(d_counts + 8)), so a synchronous call brings its
  // counts and the error bits home in ONE copy (read_counts).
  u64* d_counts = nullptr;  // 8 entries, then the ticket words
  u64* h_counts = nullptr;  // pinned, 16 entries (a mirror of the whole block)
  // synchronous calls: a one-wave kernel copies the counts into host-coherent mapped memory
  // and then stores a sequence number there, which the host polls (read_counts)
  u64* h_pub = nullptr;  // mapped host memory, 24 words: [0..16) the block, [16] the sequence
  u64* d_pub = nullptr;  // its device address
  u64 pub_seq = 0;
  u32 h_ticket[16] = {};  // the ticket words as of the last synchronous call
  u32 last_err_bits = 0;  // the error bits read_counts last failed on (0: it did not)
  Buf tmp;                // general scratch
  int join_mode = JOIN_SINGLE_PASS;  // DG_JOIN_MODE=2: two-pass count/compact variant
  int join_workers = 0;           // persistent pass-1 workgroups (0: all resident ones)
  int join_stagger = 0;           // DG_JOIN_STAGGER: the stream kernel's upper-half delay (0: none)
  // dg_apply_deltas: 0 one pass per <= 64 deltas, delta by delta where an input needs it;
  // DG_APPLY_MODE=fold: always delta by delta; =onepass: never (DG_E_INVAL instead)
  int apply_mode = 0;
  // dg_join_deltas' tree step: the incremental update (a searched thread per changed key), or
  // a rebuild (a stream over the new state) once the batch changed more than
  // rows / tree_rebuild_div keys.  DG_TREE_REBUILD=always / never / a divisor
  enum { TREE_BY_SHARE = 0, TREE_ALWAYS = 1, TREE_NEVER = 2 };
  int tree_rebuild = TREE_BY_SHARE;
  u64 tree_rebuild_div = 64;
  Buf h_stage;  // pinned staging of kernel descriptors
  Buf h_cont;   // dg_merkle_continues: per hop its descriptor and its result header (pinned; the
                // workgroups read the one and write the other in place)
  hipEvent_t ev_in = nullptr, ev_out = nullptr;  // hand-offs to the device's shared join stream
  // asynchronous calls since the last dg_engine_sync, replayed there (joins on the
  // two-pass kernels) when a single-pass join grid aborted for lack of residency
  struct Pending {
    int kind;  // 0 dg_join2_async, 1 dg_merkle_build_async
    dg_store a, b, out;
    dg_context ca, cb, out_ctx;
    const uint64_t* keys;
    uint64_t n_keys;
    uint64_t* d_counts;
    dg_merkle t;
    dg_merkle* tp;
  };
  std::vector<Pending> pending;
};

// ---- the engine's device words.  One comment per word: the kernel that writes it.

// e->ticket[0..16)
enum Ticket {
  TK_TILE = 0,    // the look-back kernels' tile ticket (join, take, kfold: left at 0 by every launch)
  TK_ERR = 1,     // error bits: a look-back timeout, an aborted join grid (join_stream.hip)
  TK_ORDER = 2,   // dg_store_check's flag (store_check_kernel)
  TK_INPUT = 3,   // a call's input-error word: the Merkle build / update (MERKLE_INPUT_ERR), the
                  // mutation count (unsorted ops), remap and mark (bad ids)
  TK_ABORT = 4,   // the join abort epoch (join_stream.hip, stripe_sums)
  TK_UNUSED = 5,
  // The Merkle kernels' arrival counter.  It is reset by the last workgroup of every build /
  // update launch, not per launch.  A launch either runs every workgroup to that reset (the
  // kernels never wait on another workgroup before arriving) or does not start at all (a
  // launch error); a kernel that faults leaves the device unusable anyway.  published_errors
  // also zeroes it whenever a call reports error bits.
  MERKLE_ARRIVE = 6,
  TAIL_ARRIVE = 7,  // dg_join_delta_home's tail kernel: every workgroup arrives
  KD_ARRIVE = 8,    // dg_join_delta's count kernel: the last workgroup scans
  MUT_ARRIVE = 9,   // dg_mutate_batch's count kernel: the last tile scans
  SPL_ARRIVE = 10,  // dg_join_delta's moved-rows copy: the last workgroup publishes
  KD_ERR = 11,      // dg_join_delta's tree input-error word (zero between calls)
  CONT_ARRIVE = 12,  // dg_merkle_continues' hop kernel: every workgroup arrives, the last resets
                     // the word and publishes (zero at creation and between launches)
};
constexpr int CONT_HOME = 18;  // h_pub words [18, 24): dg_merkle_continue_home's result header

// e->d_counts[0..8) (and their mirror e->h_counts), by the path that is running
enum JoinCount {    // the join kernels, and the splice around them
  JC_ROWS = 0,      // output rows (the join kernels; take, read, sort, the Merkle calls: their one count)
  JC_CTX = 1,       // the union context's entries (ctx_union_block)
  JC_CHANGED = 2,   // changed keys (launch_join2_changes)
  SC_TAKEN = 3,     // the state's rows of the keyset (take.hip)
  SC_BAD = 4,       // delta keys outside the keyset (splice_check_kernel)
  SC_MOVED = 5,     // u32: the edit moves rows (splice_index_kernel)
};
// (dg_join_delta's one-wait path: enum KdCount, dg_launch.h -- its kernels use the names too)
enum HomeWord {     // dg_join_delta_home's result header home[0..8) (small.hip)
  HW_FLAGS = 0,     // SMALL_FALLBACK | MERKLE_INPUT_ERR bits
  HW_CTX = 3,       // the union context's entries
  HW_EDIT = 4,      // the keyset's joined rows
  HW_TAKEN = 5,     // the state's rows of the keyset
  HW_MOVED = 6,     // rows moved
  HW_DKEYS = 7,     // the change in distinct keys
};
constexpr int TU_SHARDS = 8;  // the tree update: d_counts[0..8) are shards of the change in
                              // distinct keys (merkle_build.hip), summed by the host
enum MutateCount {  // mutate_count_kernel's last tile
  MC_KEYS = 0,      // touched keys
  MC_ROWS = 1,      // delta rows
  MC_SDOTS = 2,     // the state's dots among the delta's
};
enum MarkCount {    // mark.hip
  MK_USED = 0,      // ids used
  MK_UNKNOWN = 1,   // rows whose id is not in the table
};
enum DiffTakeCount {  // merkle_diff_take_write_kernel (the key total is JC_ROWS, as the diff's)
  DT_ROWS = 1,         // the kept keys' rows in the chosen store
};
// (the streaming store diff: enum SdCount, dg_launch.h -- its kernels use the names too)
constexpr int HC_KFOLD_FLAG = 10;  // h_counts only: kfold_pass copies its flag word here

constexpr int RETRY_WORKERS = 32;  // a join's re-run after an aborted grid (with_small_grid)

// Asynchronous calls logged for a replay at dg_engine_sync (a single-pass join grid that
// aborted for lack of residency).  A full log is settled before the next call is added.
constexpr size_t MAX_PENDING = 4096;

// The device's shared join stream, or nullptr while e is the only engine on its device.
hipStream_t shared_join_stream(dg_engine* e);

#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;  // dg_last_error's text (api_engine.hip)
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(DG_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                  __FILE__, __LINE__);                                                   \
  } while (0)

#define TRY(x)              \
  do {                      \
    int _r = (x);           \
    if (_r != DG_OK) return _r; \
  } while (0)

// ---- api_engine.hip
int set_device(dg_engine* e);
// The one grow-on-demand: at least `need` elements of `elem` bytes in *b (device memory, or
// pinned host memory), at least min_cap when it allocates; `msg` formats the element count
// of a failed allocation.  Growing waits for the stream and frees the old memory.
enum { GROW_PINNED = 1, GROW_ZERO = 2 };
int grow(dg_engine* e, Buf* b, size_t need, size_t elem, size_t min_cap, int flags, const char* msg);
int next_scan(dg_engine* e, Scan* s);
int wait_published(dg_engine* e, u64 seq);
int sync_words(dg_engine* e);
int read_counts(dg_engine* e);
int published_errors(dg_engine* e);
int settle(dg_engine* e);
Rows rows_of(const dg_store* s);
RowsOut rows_out_of(dg_store* s);
Ctx ctx_of(const dg_context* c);
MerkleT merkle_of(const dg_merkle* t);
// the five columns of n rows, src -> dst, enqueued on the engine stream
int copy_rows(dg_engine* e, const dg_store* dst, const dg_store* src, u64 n, hipMemcpyKind kind);
int check_store(const dg_store* s, const char* what);
int check_ctx(const dg_context* c, const char* what);
int check_merkle(const dg_merkle* t, const char* what);
bool pair_aligned(const void* k, const void* v, const void* t, const void* n, const void* c);
// The message of a tree input error (MERKLE_ERR_SHARD, else a bucket over 65535 rows):
// "<what>: a key outside the tree's shard" / "<what>: a bucket <holds> more than 65535 rows".
int tree_input_error(u32 bits, const char* what, const char* holds = "holds");

// ---- api_join.hip
int join2_enqueue(dg_engine* e, const dg_store* a, const dg_context* ca, const dg_store* b,
                  const dg_context* cb, const uint64_t* keys, uint64_t n_keys, dg_store* out,
                  dg_context* out_ctx, uint64_t* d_counts, void** chg = nullptr, bool force_two_pass = false);
struct Splice {  // the splice's scratch (e->spl) in use
  dg_store ak, ed;
  dg_context uctx;
  SpliceArgs sp;
  u64 n_ak = 0;
};
bool splice_wanted(const dg_engine* e, const dg_store* a, const dg_store* b, const uint64_t* keys,
                   uint64_t n_keys, const dg_store* out);
int splice_take(dg_engine* e, const dg_store* a, const dg_store* b, const uint64_t* keys, uint64_t n_keys,
                u64 uctx_cap, Splice* w, bool* ok);
int splice_edit(dg_engine* e, Splice* w, const dg_context* ca, const dg_store* b, const dg_context* cb,
                const uint64_t* keys, uint64_t n_keys, dg_context* out_ctx, bool with_changes,
                uint64_t* changed, uint64_t cap);

// ---- api_join_delta.hip
int tree_update(dg_engine* e, dg_merkle* t, const dg_store* olds, const dg_store* news, const uint64_t* keys,
                uint64_t n_keys, const char* what);

// the one-wait chain's host half around a count launch (dg_join_delta, dg_join_deltas_keyed)
int kd_fill_args(dg_engine* e, KdArgs* p, TreeScratch* ts, dg_store* state, dg_context* state_ctx,
                 const uint64_t* keys, u64 nk, const KdScratch& k, dg_store* spare, dg_merkle* tree, uint64_t* changed,
                 uint64_t cap, dg_store* rows, dg_context* ctx_out, const dg_lww_diffs* diffs);
int kd_finish_join(dg_engine* e, const KdArgs& p, const TreeScratch& ts, dg_store* state, dg_context* state_ctx,
                   dg_store* spare, dg_merkle* tree, uint64_t* n_changed, int* swapped, dg_store* rows,
                   dg_context* ctx_out, const char* what, u64* declined);

// ---- api_fold.hip
// dg_apply_deltas behind its argument checks: out <- the fold of the k deltas into (state, ctx)
int apply_deltas(dg_engine* e, const dg_store* state, const dg_context* ctx, int k, const dg_store* deltas,
                 const dg_context* dctxs, const uint64_t* const* keys, const uint64_t* n_keys, dg_store* out,
                 dg_context* out_ctx);

// ---- api_merkle.hip
int merkle_build_enqueue(dg_engine* e, const dg_store* s, dg_merkle* t, uint64_t* d_n_keys);

// ---- the grows, each with its element, minimum and message
inline int ensure_state(dg_engine* e, u64 tiles) {
  // zeroed ON the engine stream: a plain hipMemset runs on the null stream, which is not
  // ordered with a non-blocking engine stream, and could land after the next kernel has
  // already written this array.  The epoch stays monotonic: the tile-count granules
  // (e->counts) outlive this array, and a restarted epoch would make their stale values
  // read as current.
  return grow(e, &e->state, tiles, sizeof(u64), 1024, GROW_ZERO, "hipMalloc of %llu look-back granules failed");
}
inline int ensure_counts(dg_engine* e, u64 tiles) {  // zero = epoch 0: never current
  return grow(e, &e->counts, tiles, sizeof(u32), 4096, GROW_ZERO, "hipMalloc of %llu tile-count granules failed");
}
inline int ensure_tmp(dg_engine* e, size_t bytes) {
  return grow(e, &e->tmp, bytes, 1, 1 << 20, 0, "hipMalloc of %zu scratch bytes failed");
}
// Engine scratch that persists across calls (fold, spl, ubuf, sml, kdb)
inline int ensure_buf(dg_engine* e, Buf* b, size_t bytes) {
  return grow(e, b, bytes, 1, 0, 0, "hipMalloc of %zu scratch bytes failed");
}
// dg_join_delta's zero-between-calls buffer: zeroed whenever it grows and at no other time
inline int ensure_kdz(dg_engine* e, size_t bytes) {
  return grow(e, &e->kdz, bytes, 1, 0, GROW_ZERO, "hipMalloc of %zu scratch bytes failed");
}
// the full diff's two group-sum buffers (see dg_engine::diff_bsum)
inline int ensure_diff_bsum(dg_engine* e, u64 groups) {
  return grow(e, &e->diff_bsum, groups, 2 * sizeof(u64), 0, GROW_ZERO, "hipMalloc of %llu diff group sums failed");
}
inline int ensure_diff_rsum(dg_engine* e, u64 groups) {
  return grow(e, &e->diff_rsum, groups, 2 * sizeof(u64), 0, GROW_ZERO, "hipMalloc of %llu diff group sums failed");
}
// pinned host staging (kernel descriptors, digit histograms)
inline int ensure_stage(dg_engine* e, size_t bytes) {
  return grow(e, &e->h_stage, bytes, 1, 0, GROW_PINNED, "pinned staging of %zu bytes failed");
}
// dg_merkle_continues' block: k descriptors, then k result headers (u64 words)
inline int ensure_cont(dg_engine* e, size_t words) {
  return grow(e, &e->h_cont, words, sizeof(u64), 0, GROW_PINNED, "page-locked block of %llu continuation words failed");
}

// A scratch layout (dg_arena.h) in use: measured, the buffer grown to it (engine tmp with its
// minimum, any other buffer exactly), then carved from the buffer by the same `layout`.
template <class Layout>
int carve(dg_engine* e, Buf* b, Layout layout, decltype(layout(*(Arena*)nullptr))* out) {
  Arena measure;
  layout(measure);
  TRY(b == &e->tmp ? ensure_tmp(e, measure.bytes()) : ensure_buf(e, b, measure.bytes()));
  Arena real(b->p);
  *out = layout(real);
  return DG_OK;
}

// One re-run of `enqueue` on a grid small enough to find room beside other work, after a
// persistent join grid aborted for lack of residency or timed out.
template <class Fn>
int with_small_grid(dg_engine* e, Fn enqueue) {
  const int workers = e->join_workers;
  e->join_workers = RETRY_WORKERS;
  const int rc = enqueue();
  e->join_workers = workers;
  return rc;
}

// A tree update that met an input error, undone: `inverse` launches the same update with the
// opposite sign, which restores every node and count bit for bit; its own bits in *err_word
// are cleared, and the error `rc` is returned with its message kept across the wait.
template <class Launch>
int undo_tree_update(dg_engine* e, int rc, u32* err_word, Launch inverse) {
  const std::string msg = g_err;
  TRY(inverse());
  HIP_TRY(hipMemsetAsync(err_word, 0, sizeof(u32), e->stream));
  TRY(read_counts(e));
  g_err = msg;
  return rc;
}

#pragma GCC visibility pop
