// dg_jtile.h — one tile of AWLWWMap.join/3 on gfx950 (reference
// lib/delta_crdt/aw_lww_map.ex:153-209): what the stream kernel (join_stream.hip) and the
// two-pass slot kernel (join_twopass.hip) share -- the kernels' arguments, a tile's staging
// through registers into LDS, and the merge that decides keep or drop for every row.
//
// Formulation.  Both stores are sorted by the full row tuple (key, val, ts, node,
// cnt).  The joined state is the merge of the two stores filtered per row:
//
//   row of a, also in b  (same key, {v,ts} entry and dot)  -> kept   (s1 ∩ s2)
//   row of a only                                          -> kept iff dot ∉ c_b  (s1 \ c2)
//   row of b only                                          -> kept iff dot ∉ c_a  (s2 \ c1)
//   row of b equal to a row of a                           -> dropped (MapSet dedup)
//
// which is join_dot_sets/4 (:196-209) applied to every {v,ts} entry of every key;
// entries and keys that end up empty simply emit no rows (:177-181).  With an
// explicit `keys` list, rows of keys outside it are carried over right-biased
// (b's rows if b has the key, else a's), as Map.merge(Map.drop(..)) does (:185-188).
//
// Coverage (Dots.member?, :67-73) of a full-state join of two version vectors goes
// through a direct-indexed LDS table of the VVs' counters for node ids < VT (one
// ds_read per row); larger node ids and explicit dot sets use a binary search.
//
// The units of the join: join.hip (launch_join2: the routing, the partition kernel, the
// context union), join_stream.hip (the persistent single-pass kernel), join_twopass.hip
// (the slot and compact kernels), join_changes.hip (the changed keys), dg_jsplit.h (the
// merge-path split).
#pragma once
#include "dg_ctxu.h"
#include "dg_launch.h"

namespace dg {

constexpr int JB = JOIN_BLOCK;
constexpr int JI = JOIN_ITEMS;
constexpr int JT = JOIN_TILE;
static_assert(JT % 2 == 0, "even tiles (balance_tiles keeps them even)");
constexpr int JS = JT + 5;  // LDS row slots: tile rows + one neighbour on each side per store
                            // (+1: the merge's look-ahead read past the last B slot)
constexpr int VT = 64;      // VV table: node ids below this are looked up directly in LDS

struct JoinArgs {
  Rows a, b;
  Ctx ca, cb;
  const u64* keys;
  u64 n_keys;
  const u64* splits;  // merge-path split (a index) of every tile boundary (partition pass)
  u64* ksplits;       // keyed joins: first index of `keys` >= the key at every tile boundary
  u64 ntiles;
  u64 jt;     // merged positions per tile, <= JT (launch_join2 spreads the tiles evenly
              // over the grid's stripes)
  RowsOut out;
  Scan scan;  // the stream kernel's tile counts, residency flags, abort and error words
              // (scan.state holds the splits: `splits` and `ksplits` point into it)
  u64* d_count;
  unsigned short* lists;  // two-pass only: tile t's compaction list at lists[t * JT ...]
  u32* counts;            // two-pass only: kept rows per tile
  u64* chg_tmp;           // CHG: JT change-event keys per tile
  u32* chg_cnt;           // CHG: events per tile
  u32* chg_wu;            // CHG: events after the tile's first that differ from their predecessor
  u64* chg_fk;            // CHG: the tile's first and last event (tiles with events)
  u64* chg_lk;
  int stagger;            // DG_JOIN_STAGGER (0: none): the stream kernel's workgroups of the upper
                          // half of a stripe sleep this long before their first tile (STAGGER_SLEEP)
  CtxUnionArgs cu;
};

// ---- the units' launchers, as launch_join2 (join.hip) calls them
constexpr int FUSE_IT = 4;  // fused: tiles per workgroup whose splits the kernel searches itself
constexpr int CQ = (1024 + JB - 1) / JB;  // stripe counts per thread (grid <= CQ * JB)
static_assert((u64)CQ * JB + 1 <= JOIN_MAX_GRID, "start flags cover every join grid");
// join_stream.hip: the stream kernel for a join's contexts, keyset and change events, as the
// partitioned launch and as the fused one (splits searched in-kernel, one more workgroup
// for the context union)
struct StreamKernels {
  void (*part)(JoinArgs);
  void (*fused)(JoinArgs);
};
#pragma GCC visibility push(hidden)
StreamKernels stream_kernels(bool fast, bool keyed, bool chg);
u64 resident_grid(const void* k);
hipError_t launch_stream(void (*kern)(JoinArgs), u64 grid, JoinArgs& p, hipStream_t st);
// join_twopass.hip: the slot and compact kernels behind the partition launch; p.lists and
// p.counts are carved from pass_tmp (pass_layout)
hipError_t launch_two_pass(JoinArgs& p, bool fast, bool keyed, void* pass_tmp, hipStream_t st);
#pragma GCC visibility pop

namespace {

// The keyset entries a tile's keys can match (keyed joins): keys[kl, kl + km), staged in
// LDS (lds) when km <= KS -- a sync delta's few keys per tile -- else searched in global
// memory (lds == nullptr).  Membership replaces a binary search of the whole keyset per
// merged row.
constexpr int KS = 64;
struct KeySlice {
  const u64* lds;
  const u64* keys;  // keys + kl
  u64 km;
};

__device__ __forceinline__ bool key_in(const KeySlice& ks, u64 x) {
  if (ks.lds) {  // (uniform per tile) branch-free binary lifting over the staged slice
    const int km = (int)ks.km;
    int pos = 0;  // entries < x
#pragma unroll
    for (int step = KS; step >= 1; step >>= 1) {
      const int m = pos + step;
      const bool c = (m <= km) & (ks.lds[min(m, KS) - 1] < x);
      pos = c ? m : pos;
    }
    return (pos < km) & (ks.lds[min(pos, KS - 1)] == x);
  }
  return keyset_has(ks.keys, ks.km, x);
}

// VV tables: tab_a[node] / tab_b[node] = the VV's counter for node ids < VT (coalesced
// loads; the tables must have been zeroed behind a barrier).
// Returns whether this thread met a node id >= VT (a VV entry outside the tables).
__device__ __forceinline__ bool fill_vv_tables(const Ctx& ca, const Ctx& cb, u64* tab_a, u64* tab_b) {
  bool far = false;
  for (u64 i = threadIdx.x; i < ca.n; i += JB) {
    const u32 nd = ca.node[i];
    if (nd < (u32)VT) tab_a[nd] = ca.cnt[i];
    far |= nd >= (u32)VT;
  }
  for (u64 i = threadIdx.x; i < cb.n; i += JB) {
    const u32 nd = cb.node[i];
    if (nd < (u32)VT) tab_b[nd] = cb.cnt[i];
    far |= nd >= (u32)VT;
  }
  return far;
}

// The fused stream kernel fills the tables off its serial path, when neither VV has more
// than a wave's worth of entries (VVs whose node ids all lie below VT): every lane loads
// entry `lane` of both VVs at kernel entry (issue_vv), AHEAD of the first tile's loads, so
// the wait for them is a counted vmcnt that leaves the tile's loads in flight; wave 0 then
// zeroes and fills both tables by itself (fill_vv_wave0: one wave's LDS writes land in
// program order, so no barrier stands between the zeroes and the entries) while the tile
// streams in and the other waves check their splits, and the barrier behind the split
// checks publishes them.  Not the keyed kernels: they sit at 128 VGPRs, and the staged
// entries cost them scratch.
static_assert(VT == WAVE, "fill_vv_wave0 zeroes one table entry per lane");
struct VvStaged {  // one lane's entry of each VV, in registers
  u32 an, bn;
  u64 ac, bc;
};

__device__ __forceinline__ bool vv_in_wave(const Ctx& ca, const Ctx& cb) {
  return (ca.n <= (u64)WAVE) & (cb.n <= (u64)WAVE);
}

// Branch-free: a lane without an entry loads entry 0, and from a store's key column when
// the context is empty (its pointers may be null; a store with rows exists, slot_row).
__device__ __forceinline__ void issue_vv(const Ctx& ca, const Ctx& cb, const Rows& A, const Rows& B,
                                         VvStaged& v) {
  const u64 lane = threadIdx.x & (WAVE - 1);
  const u64* some = A.n ? A.key : B.key;
  const u64 na = ca.n, nb = cb.n;
  const u64 ia = lane < na ? lane : 0, ib = lane < nb ? lane : 0;
  v.an = gload(na ? ca.node : (const u32*)some, ia);
  v.ac = gload(na ? ca.cnt : some, ia);
  v.bn = gload(nb ? cb.node : (const u32*)some, ib);
  v.bc = gload(nb ? cb.cnt : some, ib);
}

// Wave 0 only, VVs of at most WAVE entries each.  Returns (wave-uniform) whether a VV has
// an entry outside the tables.
__device__ __forceinline__ bool fill_vv_wave0(const VvStaged& v, u64 na, u64 nb, u64* tab_a,
                                              u64* tab_b) {
  const u64 lane = threadIdx.x & (WAVE - 1);
  tab_a[lane] = 0;
  tab_b[lane] = 0;
  const bool ha = lane < na, hb = lane < nb;
  if (ha & (v.an < (u32)VT)) tab_a[v.an] = v.ac;
  if (hb & (v.bn < (u32)VT)) tab_b[v.bn] = v.bc;
  return __ballot((ha & (v.an >= (u32)VT)) | (hb & (v.bn >= (u32)VT))) != 0;
}

// ------------------------------------------------------------------- staging
// One staged tile: its rows (+ one neighbour on each side of each store), as 16-byte
// {key, val} and {ts, cnt} pairs plus the node column: a whole row is 3 LDS accesses
// (2 x ds_read_b128 + ds_read_b32) instead of 5, and the key-only search reads the
// low half of kv.
struct Buf {
  alignas(16) u64 kv[JS][2];
  alignas(16) u64 tc[JS][2];
  u32 node[JS];
};

__device__ __forceinline__ u64 buf_key(const Buf& s, int x) { return s.kv[x][0]; }

__device__ __forceinline__ void buf_put(Buf& s, int x, u64 key, u64 val, i64 ts, u32 node, u64 cnt) {
  typedef u64 v2u64 __attribute__((ext_vector_type(2)));
  *(v2u64*)s.kv[x] = v2u64{key, val};
  *(v2u64*)s.tc[x] = v2u64{(u64)ts, cnt};
  s.node[x] = node;
}

// Staging slot x of a tile: slot x < nat + 2 is a[a0 - 1 + x], slot x >= nat + 2 is
// b[b0 - 1 + (x - nat - 2)]; the tile has nat + nbt + 4 slots.  Returns the row to LOAD for
// the slot, for every x, so that the loads need no branch: the slot's own row where it
// exists, else a row that does -- the index clamped into the store, and the other store
// when the slot's own is empty (n == 0: its column pointers may be null; a join of two
// empty stores launches no tile kernel).  The index is below the n of the store *from_b
// names.
__device__ __forceinline__ u64 slot_row(int x, int nat, u64 a0, u64 b0, u64 na, u64 nb,
                                        bool* from_b) {
  const bool in_a = x < nat + 2;
  const i64 g = in_a ? (i64)a0 - 1 + x : (i64)b0 - 1 + (x - (nat + 2));
  const bool fb = in_a ? na == 0 : nb != 0;
  const i64 last = (i64)(fb ? nb : na) - 1;
  *from_b = fb;
  return (u64)min(max(g, (i64)0), last);
}

constexpr int SLOTS = (JS + JB - 1) / JB;

__device__ __forceinline__ Row lds_row(const Buf& s, int x) {
  typedef u64 v2u64 __attribute__((ext_vector_type(2)));
  const v2u64 kv = *(const v2u64*)s.kv[x];
  const v2u64 tc = *(const v2u64*)s.tc[x];
  Row r;
  r.key = kv.x;
  r.val = kv.y;
  r.ts = (i64)tc.x;
  r.cnt = tc.y;
  r.node = s.node[x];
  return r;
}

// Highest power of two <= JT: the first step of the binary-lifting search.
constexpr int search_top(int n) { return n <= 1 ? 1 : 2 * search_top(n / 2); }
constexpr int STOP = search_top(JT);

// Merge JI consecutive positions of the tile and decide keep/drop for each (the body
// of join_dot_sets/4 per row, see the file header).  Branch-free where it matters:
// the key search runs a fixed number of binary-lifting steps and each merge step
// selects between the a and b candidates instead of branching (divergent branches
// cost exec-mask SALU work on every path).
// CHG: also set bit k of `ev` when item k changes its key's rows (diff/3 of
// causal_crdt.ex:343-351 over `keys`): a dropped a row or a newly kept b row.
// FAST: both contexts are version vectors (LDS counter tables); KEYED: a `keys` list.
template <bool FAST, bool KEYED, bool CHG = false, bool NOFB = false>
__device__ __forceinline__ void merge_items(const Ctx& ca, const Ctx& cb, const u64* tab_a,
                                            const u64* tab_b, const KeySlice& ks,
                                            const u64 nb, const Buf& s, int nat, int nbt, u64 a0,
                                            u64 b0, u32& keep, unsigned short (&src)[JI],
                                            u32* ev = nullptr) {
  const int tid = threadIdx.x;
  const int offB = nat + 2;
  const int tt = nat + nbt;
  const int diag = min(tid * JI, tt);
  const int dend = min(diag + JI, tt);
  // Merge-path split of this thread's diagonal: first i with NOT(a[i] <= b[diag-1-i]).
  // (1) key-only: iq = first i in [lo0, hi0] with a[i].key > b[diag-1-i].key, by binary
  //     lifting (lo grows while a[m-1].key <= b[diag-m].key); slot of a[x] is 1 + x,
  //     of b[y] is offB + 1 + y.
  const int lo0 = diag > nbt ? diag - nbt : 0, hi0 = min(diag, nat);
  int lo = lo0;
#pragma unroll
  for (int step = STOP; step >= 1; step >>= 1) {
    // (both reads unconditional at a clamped index, combined bitwise: no exec-mask branch)
    const int m = lo + step;
    const int mc = min(m, hi0);
    const bool c = (m <= hi0) & (buf_key(s, mc) <= buf_key(s, offB + 1 + diag - mc));
    lo = c ? m : lo;
  }
  // (2) P(i) implies key <=, so the split is <= iq; step down while the full tuples of
  //     a[i-1] and b[diag-i] (equal keys) say a > b.  Runs of tied keys are short, and
  //     distinct keys (the common case) settle on the key columns alone.
  int i = lo;
  while (i > lo0 && buf_key(s, i) == buf_key(s, offB + 1 + diag - i)) {
    bool lt, eq;
    row_cmp_bf(lds_row(s, i), lds_row(s, offB + 1 + diag - i), lt, eq);
    if (lt | eq) break;
    i--;
  }
  int j = diag - i;
  // ra = a[i], rb = b[j] (possibly the neighbour past the tile); xa / xb are the rows
  // after them, read one step ahead so no merge step waits on LDS.  (Reads past a side's
  // end land in other slots of the buffer and are never used.)  dup: the current b row
  // equals the last a row merged before it -- ties go to a, so an a row and its equal b
  // row are adjacent and the b row is the MapSet duplicate.
  // (dup reads the last a row's key first and the whole row only under an equal key: the
  // merge is bound by its LDS reads, and in a join of replicas that hold the same keys the
  // row before a thread's first b row has another key -- config 2 36.9-37.1 against
  // 38.1-38.9 us per join, config 5 343-346 against 341 us, A/B)
  Row ra = lds_row(s, 1 + i), rb = lds_row(s, offB + 1 + j);
  bool dup = false;
  if (((a0 + (u64)i) >= 1) && buf_key(s, i) == rb.key) dup = row_eq(lds_row(s, i), rb);
  Row xa = lds_row(s, 2 + i), xb = lds_row(s, offB + 2 + j);
  keep = 0;
  if (CHG) *ev = 0;
#pragma unroll
  for (int k = 0; k < JI; k++) {
    const bool valid = diag + k < dend;
    const bool bvalid = (b0 + (u64)j) < nb;  // b[j] exists globally
    bool lt, eq;
    row_cmp_bf(ra, rb, lt, eq);
    const bool takeA = (i < nat) & ((j >= nbt) | lt | eq);
    const bool inB = bvalid & eq;
    bool kp;
    // the key is joined (in `keys`), not carried right-biased
    const bool jn = KEYED ? key_in(ks, takeA ? ra.key : rb.key) : true;
    if (FAST) {
      // Dots.member?(c_other, dot of the taken row): one LDS table read
      const u32 dn = takeA ? ra.node : rb.node;
      const u64 dc = takeA ? ra.cnt : rb.cnt;
      // (the other side's VV by field VALUES: a select between the two Ctx structs
      // would make them addressable and spill them to scratch)
      bool cov;
      if (dn < (u32)VT) {
        cov = (takeA ? tab_b : tab_a)[dn] >= dc;
      } else if (NOFB) {
        cov = dc == 0;  // no VV has an entry >= VT: Map.get(vv, dn, 0) = 0
      } else {
        const u32* vn = takeA ? opaque_ptr(cb.node) : opaque_ptr(ca.node);
        const u64* vc = takeA ? opaque_ptr(cb.cnt) : opaque_ptr(ca.cnt);
        const u64 vnn = takeA ? opaque_val(cb.n) : opaque_val(ca.n);
        cov = ctx_covers(vn, vc, vnn, 0, dn, dc);
      }
      if (KEYED) {
        // Map.merge(Map.drop(a), Map.drop(b)) for keys outside `keys`: a's rows survive
        // iff b lacks the key, b's rows always
        const bool bprev = ((b0 + (u64)j) >= 1) & (buf_key(s, offB + j) == ra.key);
        const bool bnext = bvalid & (rb.key == ra.key);
        kp = takeA ? (jn ? (inB | !cov) : !(bprev | bnext)) : (!jn | (!dup & !cov));
      } else {
        kp = takeA ? (inB || !cov) : (!dup && !cov);
      }
    } else if (takeA) {
      if (jn) {
        kp = inB || !ctx_covers(cb.node, cb.cnt, cb.n, cb.kind, ra.node, ra.cnt);
      } else {
        // Map.merge(Map.drop(a), Map.drop(b)): a's rows survive iff b lacks the key
        const bool bprev = (b0 + (u64)j) >= 1 && buf_key(s, offB + j) == ra.key;
        const bool bnext = bvalid && rb.key == ra.key;
        kp = !(bprev || bnext);
      }
    } else {
      if (jn)
        kp = !dup && !ctx_covers(ca.node, ca.cnt, ca.n, ca.kind, rb.node, rb.cnt);
      else
        kp = true;
    }
    src[k] = valid ? (unsigned short)(takeA ? 1 + i : offB + 1 + j) : (unsigned short)0;
    if (valid && kp) keep |= 1u << k;
    if (CHG && valid && jn && (takeA ? !kp : kp)) *ev |= 1u << k;
    // advance the taken side; the next row after it is read one step ahead
    // (b rows are unique and larger than every a row merged so far, so a taken b row
    // clears dup; a taken a row passes its inB on to the b row it tied with)
    dup = takeA ? inB : false;
    i += takeA ? 1 : 0;
    j += takeA ? 0 : 1;
    ra = row_sel(takeA, xa, ra);
    rb = row_sel(takeA, rb, xb);
    if (k + 1 < JI) {
      const Row nx = lds_row(s, takeA ? 2 + i : offB + 2 + j);
      xa = row_sel(takeA, nx, xa);
      xb = row_sel(takeA, xb, nx);
    }
  }
}

// Register staging of a tile: every lane issues the loads of all its slots (issue_tile)
// long before it writes them to LDS (commit_tile), so a whole tile streams in while the
// previous one is merged.  Both are straight-line code.  Loads or LDS writes under a
// per-lane `if (slot exists)` put the wait for the staged rows inside a branch, and the
// compiler, unable to prove at the loop's joins that the staging registers had no load
// pending, drained the memory pipe (vmcnt 0) before the loads of each slot: the second
// slot's loads left after the first's had landed, and the merge began after both.
struct Staged {  // one thread's share of a staged tile, in registers
  u64 k[SLOTS], v[SLOTS], c[SLOTS];
  i64 t[SLOTS];
  u32 n[SLOTS];
};

__device__ __forceinline__ void tile_geom(u64 t, u64 jt, u64 a0, u64 a1, u64 total, int* nat,
                                          int* nbt, u64* b0) {
  const u64 d0 = t * jt, d1 = min(d0 + jt, total);
  *nat = (int)(a1 - a0);
  *nbt = (int)((d1 - a1) - (d0 - a0));
  *b0 = d0 - a0;
}

// Every lane loads a row for each of its slots: slots without a row load one that exists
// (slot_row).
__device__ __forceinline__ void issue_tile(const Rows& A, const Rows& B, int nat, u64 a0, u64 b0,
                                           Staged& r) {
  const int tid = threadIdx.x;
  // (by value: a per-lane select between the two structs' fields becomes a load through a
  // selected address, see load_row_sel)
  const u64 na = opaque_val(A.n), nb = opaque_val(B.n);
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    bool fb;
    const u64 g = slot_row(tid + k * JB, nat, a0, b0, na, nb, &fb);
    const Row x = load_row_sel(A, B, fb, g);
    r.k[k] = x.key;
    r.v[k] = x.val;
    r.t[k] = x.ts;
    r.n[k] = x.node;
    r.c[k] = x.cnt;
  }
}

// Every lane writes every slot it staged, so the LDS writes -- and the wait for the staged
// rows before them -- are on every lane's path.  A slot without a row gets the row that
// issue_tile loaded in its place: the merge never uses such a slot (its validity tests:
// the global index of a neighbour, nat / nbt for the tile's ends), it held whatever an
// earlier tile left there before.  Slots past the buffer go to its last row, JS - 1, which
// no tile uses (a tile has at most JT + 4 slots).
__device__ __forceinline__ void commit_tile(const Staged& r, Buf& s) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < SLOTS; k++)
    buf_put(s, min(tid + k * JB, JS - 1), r.k[k], r.v[k], r.t[k], r.n[k], r.c[k]);
}

}  // namespace

}  // namespace dg
