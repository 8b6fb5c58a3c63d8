"""Device-resident dot stores and causal contexts, and the Engine that drives
libdeltagpu on them.

PyTorch is plumbing here: it owns HBM allocations and the stream.  Columns are
int64/int32 tensors holding the bits of the u64/i64/u32 columns of
include/deltagpu.h (u64 ids are reinterpreted, never compared in torch).
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from ._abi import DG_CTX_DOTS, DG_CTX_VV, check

_I64 = torch.int64
_I32 = torch.int32


def _ptr(t: torch.Tensor | None, ctype):
    if t is None or t.numel() == 0:
        return C.cast(C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0), ctype)
    return C.cast(C.c_void_p(t.data_ptr()), ctype)


def _ref(x):
    """byref of an optional ABI struct: None stays NULL."""
    return C.byref(x) if x is not None else None


def _np_to_dev(a: np.ndarray, dtype_view, device) -> torch.Tensor:
    a = np.ascontiguousarray(a).view(dtype_view)
    return torch.from_numpy(a.copy()).to(device, non_blocking=False)


@dataclass(eq=False)  # identity semantics: a Universe tracks stores in a WeakSet
class Store:
    """SoA dot rows on the device: key u64, val u64, ts i64, node u32, cnt u64."""

    key: torch.Tensor
    val: torch.Tensor
    ts: torch.Tensor
    node: torch.Tensor
    cnt: torch.Tensor
    n: int

    @property
    def cap(self) -> int:
        return int(self.key.numel())

    @property
    def device(self):
        return self.key.device

    @staticmethod
    def empty(cap: int, device) -> "Store":
        cap = max(int(cap), 1)
        return Store(
            torch.empty(cap, dtype=_I64, device=device),
            torch.empty(cap, dtype=_I64, device=device),
            torch.empty(cap, dtype=_I64, device=device),
            torch.empty(cap, dtype=_I32, device=device),
            torch.empty(cap, dtype=_I64, device=device),
            0,
        )

    @staticmethod
    def from_numpy(key, val, ts, node, cnt, device) -> "Store":
        n = len(key)
        if n == 0:
            return Store.empty(1, device)
        return Store(
            _np_to_dev(np.asarray(key, dtype=np.uint64), np.int64, device),
            _np_to_dev(np.asarray(val, dtype=np.uint64), np.int64, device),
            _np_to_dev(np.asarray(ts, dtype=np.int64), np.int64, device),
            _np_to_dev(np.asarray(node, dtype=np.uint32), np.int32, device),
            _np_to_dev(np.asarray(cnt, dtype=np.uint64), np.int64, device),
            n,
        )

    def to_numpy(self):
        n = self.n
        return (
            self.key[:n].cpu().numpy().view(np.uint64),
            self.val[:n].cpu().numpy().view(np.uint64),
            self.ts[:n].cpu().numpy().view(np.int64),
            self.node[:n].cpu().numpy().view(np.uint32),
            self.cnt[:n].cpu().numpy().view(np.uint64),
        )

    def abi(self) -> _abi.dg_store:
        return _abi.dg_store(self.key.data_ptr(), self.val.data_ptr(), self.ts.data_ptr(),
                             self.node.data_ptr(), self.cnt.data_ptr(), self.n, self.cap)

    def _set(self, s: _abi.dg_store):
        """Take back what a call wrote into this store's struct: its row count."""
        self.n = int(s.n)

    def swap_columns(self, other: "Store"):
        """Exchange the five column tensors with `other` (the counts stay where they are)."""
        for f in ("key", "val", "ts", "node", "cnt"):
            a, b = getattr(self, f), getattr(other, f)
            setattr(self, f, b)
            setattr(other, f, a)


@dataclass
class Context:
    """A causal context: DG_CTX_VV (version vector) or DG_CTX_DOTS (dot set)."""

    kind: int
    node: torch.Tensor
    cnt: torch.Tensor
    n: int

    @property
    def cap(self) -> int:
        return int(self.node.numel())

    @staticmethod
    def empty(kind: int, cap: int, device) -> "Context":
        cap = max(int(cap), 1)
        return Context(kind, torch.empty(cap, dtype=_I32, device=device),
                       torch.empty(cap, dtype=_I64, device=device), 0)

    @staticmethod
    def from_numpy(kind, node, cnt, device) -> "Context":
        n = len(node)
        if n == 0:
            return Context.empty(kind, 1, device)
        return Context(kind, _np_to_dev(np.asarray(node, dtype=np.uint32), np.int32, device),
                       _np_to_dev(np.asarray(cnt, dtype=np.uint64), np.int64, device), n)

    def to_numpy(self):
        return (self.node[: self.n].cpu().numpy().view(np.uint32),
                self.cnt[: self.n].cpu().numpy().view(np.uint64))

    def abi(self) -> _abi.dg_context:
        return _abi.dg_context(self.kind, 0, self.node.data_ptr(), self.cnt.data_ptr(), self.n,
                               self.cap)

    def _set(self, c: _abi.dg_context):
        """Take back what a call wrote into this context's struct: its count and kind."""
        self.n, self.kind = int(c.n), int(c.kind)


class TermHashes:
    """Device term-hash tables of a tree's rows (include/deltagpu.h dg_term_hashes):
    node_hash[node id], and the ascending non-canonical value ids with their hashes --
    `interning.Universe.term_tables()`.  Trees built with them compare across interning
    tables (replicas on other BEAM nodes)."""

    def __init__(self, node_hash, val_id, val_hash, device):
        def dev(a):
            a = np.ascontiguousarray(np.asarray(a, np.uint64))
            return _np_to_dev(a, np.int64, device) if len(a) else torch.zeros(1, dtype=_I64,
                                                                                 device=device)
        self.nh, self.vid, self.vh = dev(node_hash), dev(val_id), dev(val_hash)
        self.c = _abi.dg_term_hashes(self.nh.data_ptr(), len(node_hash), self.vid.data_ptr(),
                                     self.vh.data_ptr(), len(val_id))
        self.device = device
        self._universe = None  # set by `of`: tables that follow a Universe
        self.version = None

    @staticmethod
    def of(universe, device) -> "TermHashes":
        """The universe's current tables, uploaded once per version (cached on it)."""
        cached = getattr(universe, "_dev_terms", None)
        if cached is not None and cached[0] == universe.terms_version and cached[1] == str(device):
            return cached[2]
        th = TermHashes(*universe.term_tables(), device)
        th._universe = weakref.ref(universe)
        th.version = universe.terms_version
        universe._dev_terms = (universe.terms_version, str(device), th)
        return th

    def current(self) -> "TermHashes":
        """These tables, or their Universe's newer ones once it has interned new values or
        nodes or relabelled: ids missing from stale tables would hash as
        themselves, and the tree would stop matching a rebuild and a peer's tree.  Tables
        made from explicit arrays follow nothing and are returned as they are."""
        u = self._universe() if self._universe is not None else None
        if u is None or u.terms_version == self.version:
            return self
        return TermHashes.of(u, self.device)


@dataclass(eq=False)
class MerkleTree:
    """A device Merkle tree (include/deltagpu.h dg_merkle): its node heap, the rows per
    bucket, the term hashes its rows were hashed with (None: the ids), and the store it
    indexes (the diff recomputes key leaves from the store's rows)."""

    depth: int
    nodes: torch.Tensor
    n_keys: int = 0
    shard_bits: int = 0
    shard: int = 0
    store: Store | None = None
    counts: torch.Tensor | None = None
    terms: TermHashes | None = None
    starts: torch.Tensor | None = None  # the chunk index (dg_merkle.starts); None: not kept

    @staticmethod
    def empty(depth: int, device, shard_bits: int = 0, shard: int = 0,
              terms: TermHashes | None = None) -> "MerkleTree":
        chunks = 1 << max(depth - 11, 0)
        return MerkleTree(depth, torch.empty(2 * (1 << depth) - 1, dtype=_I64, device=device), 0,
                          shard_bits, shard, None,
                          torch.empty(max(1 << depth, 16), dtype=torch.int16, device=device), terms,
                          torch.empty(chunks + 1, dtype=_I64, device=device))

    def clone(self) -> "MerkleTree":
        return MerkleTree(self.depth, self.nodes.clone(), self.n_keys, self.shard_bits, self.shard,
                          self.store, self.counts.clone(), self.terms,
                          self.starts.clone() if self.starts is not None else None)

    def abi(self) -> _abi.dg_merkle:
        if self.terms is not None:  # follow the Universe's newest tables
            self.terms = self.terms.current()
        t = _abi.dg_merkle()
        t.depth = self.depth
        t.shard_bits = self.shard_bits
        t.shard = self.shard
        t.nodes = self.nodes.data_ptr()
        t.n_keys = self.n_keys
        t.counts = self.counts.data_ptr()
        t.terms = C.pointer(self.terms.c) if self.terms is not None else None
        t.starts = self.starts.data_ptr() if self.starts is not None else None
        return t

    def bucket_counts(self) -> np.ndarray:
        return self.counts[: 1 << self.depth].cpu().numpy().view(np.uint16)

    def root(self) -> int:
        return int(self.nodes[0].item()) & ((1 << 64) - 1)

    def level(self, lv: int) -> np.ndarray:
        return self.nodes[(1 << lv) - 1: (1 << (lv + 1)) - 1].cpu().numpy().view(np.uint64)


@dataclass(eq=False)
class MerkleCont:
    """A partial-diff continuation (dg_merkle_cont): node form (level <= depth) or leaf
    form (level == depth + 1, with the buckets its (key, leaf) pairs cover)."""

    level: int
    pos: torch.Tensor
    hash: torch.Tensor
    n: int
    bucket: torch.Tensor | None = None
    n_buckets: int = 0

    @staticmethod
    def empty(cap: int, cap_buckets: int, device) -> "MerkleCont":
        cap, cap_buckets = max(int(cap), 1), max(int(cap_buckets), 1)
        return MerkleCont(0, torch.empty(cap, dtype=_I64, device=device),
                          torch.empty(cap, dtype=_I64, device=device), 0,
                          torch.empty(cap_buckets, dtype=_I64, device=device), 0)

    @property
    def leaf(self) -> bool:
        return self.n_buckets > 0

    def abi(self) -> _abi.dg_merkle_cont:
        c = _abi.dg_merkle_cont()
        c.level = self.level
        c.pos = self.pos.data_ptr()
        c.hash = self.hash.data_ptr()
        c.n = self.n
        c.cap = int(self.pos.numel())
        c.bucket = self.bucket.data_ptr() if self.bucket is not None else None
        c.n_buckets = self.n_buckets
        c.cap_buckets = int(self.bucket.numel()) if self.bucket is not None else 0
        return c

    def _set(self, c: _abi.dg_merkle_cont):
        self.level, self.n, self.n_buckets = int(c.level), int(c.n), int(c.n_buckets)


def fold_roots(roots) -> int:
    """dg_merkle_fold_roots: the unsharded root from the 2^b shard roots (shard order)."""
    lib = _abi.load()
    r = np.ascontiguousarray(np.asarray(roots, dtype=np.uint64))
    b = int(len(r)).bit_length() - 1
    if len(r) != 1 << b:
        raise ValueError("fold_roots needs a power-of-two number of shard roots")
    out = C.c_uint64()
    check(lib.dg_merkle_fold_roots(r.ctypes.data_as(_abi.P64), b, C.byref(out)))
    return int(out.value)


class Engine:
    """One libdeltagpu engine (one HIP stream) on one device."""

    def __init__(self, device=None, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("libdeltagpu needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _abi.load()
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                           torch.device(device).index or 0)
        self.device = dev
        if stream is None:
            # a dedicated stream: the legacy null stream (handle 0) would be ambiguous
            # at the C-ABI, where NULL means "create one"
            stream = torch.cuda.Stream(device=dev)
        self.stream = stream
        h = C.c_void_p()
        check(self.lib.dg_engine_create(dev.index, C.c_void_p(stream.cuda_stream), C.byref(h)))
        self.h = h
        self._d_counts = torch.zeros(8, dtype=_I64, device=dev)

    def _order(self):
        """Make the engine stream wait for work already queued on torch's current stream
        (uploads of the inputs), so a call never reads half-written tensors."""
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            # one reused event (Stream.wait_stream creates a new one per call)
            if getattr(self, "_order_ev", None) is None:
                self._order_ev = torch.cuda.Event()
            self._order_ev.record(cur)
            self.stream.wait_event(self._order_ev)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_home", None) is not None:
                self.lib.dg_host_free(self.h, self._home)
                self._home = None
            self.lib.dg_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.dg_engine_sync(self.h))

    # ---------------------------------------------------------------- join
    def _keys(self, keys: torch.Tensor | None):
        """(pointer, n) of a `keys` argument: None -> NULL (every key); an empty tensor
        -> a valid pointer with n = 0 (no key -- an empty tensor's data_ptr() is 0,
        which the C-ABI would read as NULL)."""
        if keys is None:
            return None, 0
        if keys.numel() == 0:
            if getattr(self, "_no_keys", None) is None:
                self._no_keys = torch.zeros(1, dtype=_I64, device=self.device)
            return _ptr(self._no_keys, _abi.P64), 0
        return _ptr(keys, _abi.P64), int(keys.numel())

    def _keysets(self, keys):
        """(kp, kn, keepalive) of a list of keysets -- the `void*[k]` and `uint64[k]` pair of
        the batch calls: None for the whole list -> NULL, NULL; an element goes by `_keys`'
        rule (None: every key; an empty tensor: a join or take over no key, not a full-state
        one).  `keepalive` owns the memory `kn` points into and the keysets themselves."""
        if keys is None:
            return None, None, ()
        ptrs = [C.cast(self._keys(t)[0], C.c_void_p) if t is not None else None for t in keys]
        kp = (C.c_void_p * max(len(keys), 1))(*ptrs)
        kn_np = np.array([int(t.numel()) if t is not None else 0 for t in keys] or [0], np.uint64)
        return kp, kn_np.ctypes.data_as(_abi.P64), (kn_np, keys)

    @staticmethod
    def _structs(items, ctype):
        """The `ctype[k]` array of the ABI structs of k stores or contexts (k = 0: one zeroed
        element, so that the array has an address)."""
        return (ctype * max(len(items), 1))(*[x.abi() for x in items])

    def _outputs(self, out, out_ctx, n_rows, n_ctx):
        """A join's outputs: the caller's, or fresh ones of the given sizes."""
        if out is None:
            out = Store.empty(n_rows, self.device)
        if out_ctx is None:
            out_ctx = Context.empty(DG_CTX_VV, n_ctx, self.device)
        return out, out_ctx

    @staticmethod
    def _commit_join(state, state_ctx, spare, tree, ss, sc, t, swapped):
        """What every resident join does behind the library's call: when the result landed
        in `spare`, the two Store objects exchange their columns (`state` always holds the
        joined rows, `spare` the old ones with n = 0); the counts come back from the structs
        and `tree` indexes `state`.  `state_ctx` None: a call that leaves the context alone
        (replace_keysets)."""
        if swapped:
            state.swap_columns(spare)
            spare.n = 0
        state._set(ss)
        if state_ctx is not None:
            state_ctx._set(sc)
        if tree is not None:
            tree.n_keys = int(t.n_keys) & ((1 << 64) - 1)
            tree.store = state

    def join2(self, a: Store, ca: Context, b: Store, cb: Context, keys: torch.Tensor | None = None,
              out: Store | None = None, out_ctx: Context | None = None):
        self._order()
        out, out_ctx = self._outputs(out, out_ctx, a.n + b.n, ca.n + cb.n)
        so, co = out.abi(), out_ctx.abi()
        sa, sb, xa, xb = a.abi(), b.abi(), ca.abi(), cb.abi()
        kp, nk = self._keys(keys)
        check(self.lib.dg_join2(self.h, C.byref(sa), C.byref(xa), C.byref(sb), C.byref(xb),
                                kp, nk, C.byref(so), C.byref(co)))
        out._set(so)
        out_ctx._set(co)
        return out, out_ctx

    def join2_changes(self, a: Store, ca: Context, b: Store, cb: Context,
                      keys: torch.Tensor | None = None, out: Store | None = None,
                      out_ctx: Context | None = None):
        """join/3 plus CausalCrdt's changed-key diff (diff/3, causal_crdt.ex:343-351):
        returns (out, out_ctx, changed) with `changed` the ascending device int64 tensor
        of the keys (of `keys`, or all) whose rows in `out` differ from those in `a`."""
        self._order()
        out, out_ctx = self._outputs(out, out_ctx, a.n + b.n, ca.n + cb.n)
        cap = max(a.n + b.n, 1)
        changed = torch.empty(cap, dtype=_I64, device=self.device)
        so, co = out.abi(), out_ctx.abi()
        sa, sb, xa, xb = a.abi(), b.abi(), ca.abi(), cb.abi()
        kp, nk = self._keys(keys)
        n = C.c_uint64(0)
        check(self.lib.dg_join2_changes(self.h, C.byref(sa), C.byref(xa), C.byref(sb), C.byref(xb),
                                        kp, nk, C.byref(so), C.byref(co), _ptr(changed, _abi.P64),
                                        cap, C.byref(n)))
        out._set(so)
        out_ctx._set(co)
        return out, out_ctx, changed[: n.value]

    def join2_async(self, a: Store, ca: Context, b: Store, cb: Context, out: Store,
                    out_ctx: Context, keys: torch.Tensor | None = None, d_counts=None):
        """Enqueue the join; counts land in d_counts[0:2] (device)."""
        self._order()
        if d_counts is None:
            d_counts = self._d_counts
        so, co = out.abi(), out_ctx.abi()
        sa, sb, xa, xb = a.abi(), b.abi(), ca.abi(), cb.abi()
        kp, nk = self._keys(keys)
        check(self.lib.dg_join2_async(self.h, C.byref(sa), C.byref(xa), C.byref(sb), C.byref(xb),
                                      kp, nk, C.byref(so), C.byref(co), _ptr(d_counts, _abi.P64)))
        out_ctx.kind = int(co.kind)
        return d_counts

    def prepare_join2(self, a: Store, ca: Context, b: Store, cb: Context, out: Store,
                      out_ctx: Context, d_counts: torch.Tensor, keys: torch.Tensor | None = None):
        """Pre-marshal one join for repeated asynchronous launches (benchmark loops):
        returns a zero-argument callable that enqueues dg_join2_async."""
        args = [a.abi(), ca.abi(), b.abi(), cb.abi(), out.abi(), out_ctx.abi()]
        refs = [C.byref(x) for x in args]
        kp, nk = self._keys(keys)
        dp = _ptr(d_counts, _abi.P64)
        f, h = self.lib.dg_join2_async, self.h

        def launch():
            check(f(h, refs[0], refs[1], refs[2], refs[3], kp, nk, refs[4], refs[5], dp))

        # the device memory the raw pointers name stays alive as long as the callable
        launch._keep = (a, ca, b, cb, out, out_ctx, args, keys, d_counts)
        launch.out_ctx_abi = args[5]  # the dg_context each launch fills in (its kind)
        return launch

    def joink(self, stores, ctxs, out: Store | None = None, out_ctx: Context | None = None):
        self._order()
        k = len(stores)
        arr_s, arr_c = self._structs(stores, _abi.dg_store), self._structs(ctxs, _abi.dg_context)
        out, out_ctx = self._outputs(out, out_ctx, sum(s.n for s in stores), sum(c.n for c in ctxs))
        so, co = out.abi(), out_ctx.abi()
        check(self.lib.dg_joink(self.h, k, arr_s, arr_c, C.byref(so), C.byref(co)))
        out._set(so)
        out_ctx._set(co)
        return out, out_ctx

    def prepare_apply_deltas(self, state: Store, ctx: Context, deltas, dctxs, keys, out: Store,
                             out_ctx: Context):
        """Pre-marshal one dg_apply_deltas call for repeated use (benchmark loops, a
        replica re-applying the same batch shape): returns a zero-argument callable that
        runs it and returns (out, out_ctx)."""
        k = len(deltas)
        arr_s, arr_c = self._structs(deltas, _abi.dg_store), self._structs(dctxs, _abi.dg_context)
        kp, kn, keep = self._keysets(keys)
        ss, xs, so, co = state.abi(), ctx.abi(), out.abi(), out_ctx.abi()
        refs = (C.byref(ss), C.byref(xs), C.byref(so), C.byref(co))
        f, h = self.lib.dg_apply_deltas, self.h

        def run():
            self._order()
            check(f(h, refs[0], refs[1], k, arr_s, arr_c, kp, kn, refs[2], refs[3]))
            out.n = int(so.n)
            out_ctx.n = int(co.n)
            out_ctx.kind = int(co.kind)
            return out, out_ctx

        run._keep = (arr_s, arr_c, kp, kn, keep, ss, xs, so, co, state, ctx, deltas, dctxs)
        return run

    def apply_deltas(self, state: Store, ctx: Context, deltas, dctxs, keys=None,
                     out: Store | None = None, out_ctx: Context | None = None):
        """CausalCrdt's delta application (causal_crdt.ex:383-384): fold of
        join(state, deltas[i], keys[i]); keys[i] a sorted unique device int64 tensor of
        key ids, or None for a full-state join of that delta."""
        out, out_ctx = self._outputs(out, out_ctx, state.n + sum(d.n for d in deltas),
                                     ctx.n + sum(c.n for c in dctxs))
        return self.prepare_apply_deltas(state, ctx, deltas, dctxs, keys, out, out_ctx)()

    def take_keys(self, s: Store, keys: torch.Tensor, out: Store | None = None) -> Store:
        """Map.take(value, keys) of a sync delta (causal_crdt.ex:324-335): the rows of `s`
        whose key is in `keys` (ascending unique device int64), in store order."""
        self._order()
        kp, nk = self._keys(keys)
        ss = s.abi()
        if out is None:
            # a sync delta holds a few rows per key: room for four (an output of the whole
            # store's size -- 450 MB at config 4 -- cost more than the call); more rows than
            # that: the call reports DG_E_CAPACITY and runs again into a store-sized output
            out = Store.empty(min(max(s.n, 1), max(4 * int(nk), 256)), self.device)
            so = out.abi()
            rc = self.lib.dg_take_keys(self.h, C.byref(ss), kp, nk, C.byref(so))
            if rc == _abi.DG_E_CAPACITY and out.cap < s.n:
                out = Store.empty(max(s.n, 1), self.device)
                so = out.abi()
                rc = self.lib.dg_take_keys(self.h, C.byref(ss), kp, nk, C.byref(so))
            check(rc)
        else:
            so = out.abi()
            check(self.lib.dg_take_keys(self.h, C.byref(ss), kp, nk, C.byref(so)))
        out._set(so)
        return out

    def take_keysets(self, s: Store, keysets, out: Store | None = None, cap_keys: int | None = None):
        """Map.take(value, keys_j) for k <= 64 keysets out of one pass (dg_take_keysets): every
        distinct key located once, every row copied once.  `keysets`: ascending unique device
        int64 tensors.  Returns (ukeys, masks, offs, out): the union of the keysets, per union
        key the bit mask of the keysets that hold it, offs[i]..offs[i + 1] its rows in `out`
        (offs has len(ukeys) + 1 entries), and `out` the union's rows in store order.  Keyset
        j's take is the concatenation of the ranges of the keys whose mask has bit j.
        With `out` and `cap_keys` left to the call, a result that does not fit is taken again
        at the sizes the call reports; given ones are used as they are, and a CapacityError
        then carries the needed sizes as `.n_ukeys` and `.n_rows`."""
        self._order()
        k = len(keysets)
        kp, kn, _keep = self._keysets(keysets)
        m = sum(int(t.numel()) for t in keysets)
        own_out, own_cap = out is None, cap_keys is None
        ss = s.abi()
        for attempt in range(2):
            if cap_keys is None:
                cap_keys = m
            if out is None:
                out = Store.empty(min(max(s.n, 1), max(4 * m, 256)), self.device)
            ukeys = torch.empty(max(cap_keys, 1), dtype=_I64, device=self.device)
            masks = torch.empty(max(cap_keys, 1), dtype=_I64, device=self.device)
            offs = torch.empty(cap_keys + 1, dtype=_I64, device=self.device)
            so = out.abi()
            nu = C.c_uint64(0)
            rc = self.lib.dg_take_keysets(self.h, C.byref(ss), k, kp, kn, _ptr(ukeys, _abi.P64),
                                          _ptr(masks, _abi.P64), _ptr(offs, _abi.P64), cap_keys, C.byref(nu),
                                          C.byref(so))
            if rc == _abi.DG_E_CAPACITY:
                if attempt == 0 and (own_out or int(so.n) <= out.cap) and (own_cap or nu.value <= cap_keys):
                    if int(so.n) > out.cap:
                        out = Store.empty(int(so.n), self.device)
                    if nu.value > cap_keys:
                        cap_keys = int(nu.value)
                    continue
                try:
                    check(rc)
                except _abi.CapacityError as err:
                    err.n_ukeys, err.n_rows = int(nu.value), int(so.n)
                    raise
            check(rc)
            break
        out._set(so)
        n = int(nu.value)
        return ukeys[:n], masks[:n], offs[:n + 1], out

    def replace_keysets(self, state: Store, keysets, row_stores, spare: Store,
                        tree: MerkleTree | None = None):
        """k journal records applied to a resident state in one splice (dg_replace_keysets):
        for every key of `keysets[j]` (ascending unique device int64) the state's rows become
        `row_stores[j]`'s rows of that key (none: the key is removed); the last record naming
        a key wins, every other row stays, `tree` (indexing `state`) follows.  The records are
        laid end to end here and the offsets computed; the swap is committed as after
        join_delta.  Returns (number of union keys, swapped)."""
        self._order()
        k = len(keysets)
        if len(row_stores) != k:
            raise ValueError("replace_keysets: one row store per keyset")
        key_off = np.zeros(k + 1, np.int64)
        row_off = np.zeros(k + 1, np.int64)
        np.cumsum(np.array([int(t.numel()) for t in keysets], np.int64), out=key_off[1:])
        np.cumsum(np.array([s.n for s in row_stores], np.int64), out=row_off[1:])
        m, n = int(key_off[k]), int(row_off[k])
        keys_cat = (torch.cat([t.reshape(-1) for t in keysets]) if m else
                    torch.zeros(1, dtype=_I64, device=self.device))
        rows_cat = Store.empty(n, self.device)
        with_rows = [s for s in row_stores if s.n]
        for f in ("key", "val", "ts", "node", "cnt"):
            if with_rows:
                getattr(rows_cat, f)[:n].copy_(torch.cat([getattr(s, f)[: s.n] for s in with_rows]))
        rows_cat.n = n
        return self.replace_keysets_cat(state, keys_cat, key_off, rows_cat, row_off, spare, tree)

    def replace_keysets_cat(self, state: Store, keys_cat: torch.Tensor, key_off, rows_cat: Store, row_off,
                            spare: Store, tree: MerkleTree | None = None):
        """replace_keysets on records already laid end to end (what a journal reader has):
        `keys_cat` (device int64) and `rows_cat` with their k + 1 host offsets each."""
        k = len(key_off) - 1
        d_koff = torch.from_numpy(np.ascontiguousarray(key_off, np.int64)).to(self.device)
        d_roff = torch.from_numpy(np.ascontiguousarray(row_off, np.int64)).to(self.device)
        self._order()  # (uploads and concatenations ran on torch's stream)
        ss, sr, sp = state.abi(), rows_cat.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        nu = C.c_uint64(0)
        sw = C.c_int(0)
        check(self.lib.dg_replace_keysets(self.h, C.byref(ss), k, _ptr(keys_cat, _abi.P64), _ptr(d_koff, _abi.P64),
                                          C.byref(sr), _ptr(d_roff, _abi.P64), C.byref(sp), _ref(t), C.byref(nu),
                                          C.byref(sw)))
        self._commit_join(state, None, spare, tree, ss, None, t, sw.value)
        return int(nu.value), bool(sw.value)

    def mutate_batch(self, state: Store, ctx: Context, node: int, kind: torch.Tensor,
                     key: torch.Tensor, val: torch.Tensor, ts: torch.Tensor,
                     add_rank: torch.Tensor, n_adds: int):
        """A batch of add/remove ops by `node` as one delta (aw_lww_map.ex:99-146):
        device arrays sorted by key (batch order within a key); kind uint8 (1 add),
        add_rank = adds before the op in batch order.  Returns (delta Store, its dot-list
        Context, touched keys) -- join the delta with those keys."""
        self._order()
        m = int(key.numel())
        out = Store.empty(max(m, 1), self.device)
        keys = torch.empty(max(m, 1), dtype=_I64, device=self.device)
        nk = C.c_uint64(0)
        ss, xs, so = state.abi(), ctx.abi(), out.abi()
        args = [_ptr(kind, C.c_void_p) if m else None, _ptr(key, _abi.P64), _ptr(val, _abi.P64),
                _ptr(ts, _abi.PI64), _ptr(add_rank, _abi.P64)]
        for cap in (8 * m + n_adds + 1, state.n + n_adds + 1):
            dots = Context.empty(DG_CTX_DOTS, cap, self.device)
            xd = dots.abi()
            rc = self.lib.dg_mutate_batch(self.h, C.byref(ss), C.byref(xs), node, m, *args, n_adds,
                                          C.byref(so), C.byref(xd), _ptr(keys, _abi.P64),
                                          max(m, 1), C.byref(nk))
            if rc != _abi.DG_E_CAPACITY:
                break
        check(rc)
        out._set(so)
        dots._set(xd)
        return out, dots, keys[: nk.value]

    # ---------------------------------------------------------------- contexts
    def context_union(self, a: Context, b: Context, out: Context | None = None) -> Context:
        self._order()
        if out is None:
            out = Context.empty(DG_CTX_VV, a.n + b.n, self.device)
        xa, xb, xo = a.abi(), b.abi(), out.abi()
        check(self.lib.dg_context_union(self.h, C.byref(xa), C.byref(xb), C.byref(xo)))
        out._set(xo)
        return out

    def compress_dots(self, dots: Context, out: Context | None = None) -> Context:
        self._order()
        if out is None:
            out = Context.empty(DG_CTX_VV, dots.n, self.device)
        xa, xo = dots.abi(), out.abi()
        check(self.lib.dg_compress_dots(self.h, C.byref(xa), C.byref(xo)))
        out._set(xo)
        return out

    # ---------------------------------------------------------------- read
    def read_lww(self, s: Store, keys: torch.Tensor | None = None):
        self._order()
        cap = max(s.n, 1)
        ok = torch.empty(cap, dtype=_I64, device=self.device)
        ov = torch.empty(cap, dtype=_I64, device=self.device)
        n = C.c_uint64()
        ss = s.abi()
        kp, nk = self._keys(keys)
        check(self.lib.dg_read_lww(self.h, C.byref(ss), kp, nk, _ptr(ok, _abi.P64),
                                   _ptr(ov, _abi.P64), cap, C.byref(n)))
        return ok[: n.value], ov[: n.value]

    # ---------------------------------------------------------------- merkle
    def merkle_build(self, s: Store, depth: int, tree: MerkleTree | None = None,
                     shard_bits: int = 0, shard: int = 0,
                     terms: TermHashes | None = None) -> MerkleTree:
        """MerkleMap over every key of `s` (or of its key-hash shard); `terms`: hash the
        rows' terms instead of their ids (a given `tree` keeps its own)."""
        self._order()
        if tree is None or tree.depth != depth:
            tree = MerkleTree.empty(depth, self.device, shard_bits, shard,
                                    terms if terms is not None else (tree.terms if tree else None))
        elif terms is not None:
            tree.terms = terms
        tree.shard_bits, tree.shard = shard_bits, shard
        t = tree.abi()
        ss = s.abi()
        check(self.lib.dg_merkle_build(self.h, C.byref(ss), C.byref(t)))
        tree.n_keys = int(t.n_keys)
        tree.store = s
        return tree

    def prepare_merkle_build(self, s: Store, tree: MerkleTree, d_counts: torch.Tensor):
        """Pre-marshal one dg_merkle_build_async (benchmark loops): a zero-argument
        callable that enqueues the build on the engine stream."""
        args = [s.abi(), tree.abi()]
        refs = [C.byref(x) for x in args]
        dp = _ptr(d_counts, _abi.P64)
        f, h = self.lib.dg_merkle_build_async, self.h

        def launch():
            check(f(h, refs[0], refs[1], dp))

        launch._keep = (args, d_counts, s, tree)
        tree.store = s
        return launch

    def join_delta(self, state: Store, state_ctx: Context, delta: Store, delta_ctx: Context,
                   keys: torch.Tensor, spare: Store, tree: MerkleTree | None = None,
                   changed: torch.Tensor | None = None, rows: Store | None = None):
        """CausalCrdt.update_state_with_delta on a device-resident state
        (causal_crdt.ex:383-404, dg_join_delta): `state` and `state_ctx` become the keyed
        join with the sync delta, `tree` (indexing `state`) is updated for the changed keys.
        In place when every joined key keeps its row count; otherwise the result lands in
        `spare` and the two Store objects exchange their columns (so `state` always holds
        the joined rows).  `rows` (optional): receives the changed keys' joined rows
        (dg_join_delta_rows, what on_diffs reads).  Returns (changed keys, swapped)."""
        self._order()
        if changed is None:
            changed = torch.empty(max(int(keys.numel()), 1), dtype=_I64, device=self.device)
        ss, sc, sd, cd, sp = state.abi(), state_ctx.abi(), delta.abi(), delta_ctx.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        kp, nk = self._keys(keys)
        n = C.c_uint64(0)
        sw = C.c_int(0)
        args = (self.h, C.byref(ss), C.byref(sc), C.byref(sd), C.byref(cd), kp, nk, C.byref(sp),
                _ref(t), _ptr(changed, _abi.P64), int(changed.numel()), C.byref(n), C.byref(sw))
        if rows is None:
            check(self.lib.dg_join_delta(*args))
        else:
            ro = rows.abi()
            check(self.lib.dg_join_delta_rows(*args, C.byref(ro)))
            rows._set(ro)
        self._commit_join(state, state_ctx, spare, tree, ss, sc, t, sw.value)
        return changed[: n.value], bool(sw.value)

    def _diffs(self, cap: int):
        """Device arrays for a dg_lww_diffs of `cap` entries and their struct."""
        cap = max(int(cap), 1)
        ov = torch.empty(cap, dtype=_I64, device=self.device)
        nv = torch.empty(cap, dtype=_I64, device=self.device)
        fl = torch.empty(cap, dtype=torch.uint8, device=self.device)
        return ov, nv, fl, _abi.dg_lww_diffs(ov.data_ptr(), nv.data_ptr(), fl.data_ptr(), cap)

    def read_diff(self, old: Store, new: Store, keys: torch.Tensor):
        """read/2 of `keys` (device int64, any order) on two stores side by side
        (dg_read_diff; diffs_to_callback/3, causal_crdt.ex:364-373): (old_val, new_val,
        flags) per key -- value ids (0 where absent) and DG_DIFF_OLD | DG_DIFF_NEW bits."""
        self._order()
        n = int(keys.numel())
        ov, nv, fl, d = self._diffs(n)
        so, sn = old.abi(), new.abi()
        kp, nk = self._keys(keys)
        check(self.lib.dg_read_diff(self.h, C.byref(so), C.byref(sn), kp, nk, C.byref(d)))
        return ov[:n], nv[:n], fl[:n]

    def join_delta_diffs(self, state: Store, state_ctx: Context, delta: Store, delta_ctx: Context,
                         keys: torch.Tensor, spare: Store, tree: MerkleTree | None = None,
                         changed: torch.Tensor | None = None, rows: Store | None = None,
                         diffs: _abi.dg_lww_diffs | None = None, ctx_out: Context | None = None):
        """join_delta plus, for every changed key, its LWW read before and after the join
        (dg_join_delta_diffs: what on_diffs compares, served from the resident state whose
        old rows the join overwrites).  Returns (changed keys, old_val, new_val, flags,
        swapped), entry i of the three describing changed[i].  `diffs`: the caller's own
        arrays (e.g. page-locked memory from dg_host_alloc) receive them instead, and the
        three returned arrays are None.  `rows` / `ctx_out` (optional): the changed keys'
        joined rows and a copy of the joined context, as dg_join_delta_out gives them."""
        self._order()
        if changed is None:
            changed = torch.empty(max(int(keys.numel()), 1), dtype=_I64, device=self.device)
        cap = int(changed.numel())
        own = diffs is None
        if own:
            ov, nv, fl, d = self._diffs(cap)
        else:
            ov = nv = fl = None
            d = diffs
        ss, sc, sd, cd, sp = state.abi(), state_ctx.abi(), delta.abi(), delta_ctx.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        ro = rows.abi() if rows is not None else None
        co = ctx_out.abi() if ctx_out is not None else None
        kp, nk = self._keys(keys)
        n = C.c_uint64(0)
        sw = C.c_int(0)
        check(self.lib.dg_join_delta_diffs(
            self.h, C.byref(ss), C.byref(sc), C.byref(sd), C.byref(cd), kp, nk, C.byref(sp),
            _ref(t), _ptr(changed, _abi.P64), cap, C.byref(n), C.byref(sw), _ref(ro), _ref(co), C.byref(d)))
        if rows is not None:
            rows._set(ro)
        if ctx_out is not None:
            ctx_out._set(co)
        self._commit_join(state, state_ctx, spare, tree, ss, sc, t, sw.value)
        nch = int(n.value)
        if own and d.cap == 0 and nch:
            # the gather behind a committed join failed (deltagpu.h): the old rows survive
            # only where the join went through the spare store
            if not sw.value:
                raise _abi.DeltaGpuError(_abi.DG_E_DEVICE, "the join applied, but its diffs were not "
                                         "gathered and the old rows are overwritten")
            spare.n = int(sp.n)  # the old rows count again while they are read
            ov, nv, fl = self.read_diff(spare, state, changed[:nch])
            spare.n = 0
        if not own:
            return changed[:nch], None, None, None, bool(sw.value)
        return changed[:nch], ov[:nch], nv[:nch], fl[:nch], bool(sw.value)

    def store_diff(self, old: Store, new: Store, want_rows: bool = False, want_diffs: bool = False,
                   changed: torch.Tensor | None = None, rows: Store | None = None):
        """The streaming diff of two stores (dg_store_diff): every key whose rows differ
        between `old` and `new`, ascending.  Returns the changed keys alone, or a tuple
        (changed[, rows][, (old_val, new_val, flags)]) with the changed keys' rows of `new`
        (want_rows) and their LWW reads on either side (want_diffs).  `changed` / `rows`: the
        caller's own buffers (too small a `changed` raises CapacityError)."""
        self._order()
        if changed is None:
            changed = torch.empty(max(old.n + new.n, 1), dtype=_I64, device=self.device)
        cap = int(changed.numel())
        if want_rows and rows is None:
            rows = Store.empty(max(new.n, 1), self.device)
        ro = rows.abi() if want_rows else None
        if want_diffs:
            ov, nv, fl, d = self._diffs(cap)
        so, sn = old.abi(), new.abi()
        n = C.c_uint64(0)
        check(self.lib.dg_store_diff(self.h, C.byref(so), C.byref(sn), _ptr(changed, _abi.P64), cap, C.byref(n),
                                     _ref(ro), C.byref(d) if want_diffs else None))
        nch = int(n.value)
        out = [changed[:nch]]
        if want_rows:
            rows._set(ro)
            if rows.n > rows.cap:
                raise _abi.CapacityError(_abi.DG_E_CAPACITY, f"store_diff: {rows.n} rows > cap {rows.cap}")
            out.append(rows)
        if want_diffs:
            out.append((ov[:nch], nv[:nch], fl[:nch]))
        return out[0] if len(out) == 1 else tuple(out)

    def join_deltas(self, state: Store, state_ctx: Context, deltas, dctxs, keys, spare: Store,
                    tree: MerkleTree | None = None, changed: torch.Tensor | None = None,
                    rows: Store | None = None, diffs: _abi.dg_lww_diffs | None = None,
                    ctx_out: Context | None = None):
        """CausalCrdt.update_state_with_delta for a batch of deltas on a device-resident state
        (dg_join_deltas): `state` and `state_ctx` become the fold of join(state, deltas[i],
        keys[i]) (keys as for apply_deltas), `tree` follows, and the changed keys are the
        batch's NET change with their LWW reads before and after the batch.  With at least one
        delta the result lands in `spare` and the two Store objects exchange their columns;
        `spare` then holds the old rows (n = 0, as after join_delta).  Returns what
        join_delta_diffs returns: (changed keys, old_val, new_val, flags, swapped)."""
        return self._join_batch(False, state, state_ctx, deltas, dctxs, keys, spare, tree, changed, rows, diffs,
                                ctx_out, True)

    def join_deltas_keyed(self, state: Store, state_ctx: Context, deltas, dctxs, keys, spare: Store,
                          tree: MerkleTree | None = None, changed: torch.Tensor | None = None,
                          rows: Store | None = None, diffs: _abi.dg_lww_diffs | None = None,
                          ctx_out: Context | None = None, want_diffs: bool = True):
        """join_deltas at the cost of the keys the batch names (dg_join_deltas_keyed): a thread
        per key of the keysets' union, in place when every union key keeps its row count
        (swapped False, `spare` untouched), else through `spare` as join_delta.  Returns
        join_deltas' tuple, or None when the library declined (DG_KEYED_FALLBACK: nothing was
        touched -- call join_deltas).  want_diffs=False: the library computes no diffs (the
        three diff arrays of the tuple are None)."""
        return self._join_batch(True, state, state_ctx, deltas, dctxs, keys, spare, tree, changed, rows, diffs,
                                ctx_out, want_diffs)

    def _join_batch(self, keyed, state, state_ctx, deltas, dctxs, keys, spare, tree, changed, rows, diffs,
                    ctx_out, want_diffs):
        """The marshalling join_deltas and join_deltas_keyed share, and the commit behind the
        call (`_commit_join`)."""
        self._order()
        k = len(deltas)
        arr_s, arr_c = self._structs(deltas, _abi.dg_store), self._structs(dctxs, _abi.dg_context)
        kp, kn, _keep = self._keysets(keys)
        if changed is None:
            full = keys is None or any(t is None for t in keys)
            bound = sum(d.n for d in deltas) + (state.n if full else sum(int(t.numel()) for t in keys))
            changed = torch.empty(max(bound, 1), dtype=_I64, device=self.device)
        cap = int(changed.numel())
        own = want_diffs and diffs is None
        ov = nv = fl = None
        d = diffs if want_diffs else None
        if own:
            ov, nv, fl, d = self._diffs(cap)
        ss, sc, sp = state.abi(), state_ctx.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        ro = rows.abi() if rows is not None else None
        co = ctx_out.abi() if ctx_out is not None else None
        n = C.c_uint64(0)
        args = (self.h, C.byref(ss), C.byref(sc), k, arr_s, arr_c, kp, kn, C.byref(sp), _ref(t),
                _ptr(changed, _abi.P64), cap, C.byref(n), _ref(ro), _ref(co), _ref(d))
        if keyed:
            sw = C.c_int(0)
            rc = self.lib.dg_join_deltas_keyed(*args, C.byref(sw))
            if rc == _abi.DG_KEYED_FALLBACK:
                return None
            check(rc)
            swapped = bool(sw.value)
        else:
            check(self.lib.dg_join_deltas(*args))
            swapped = k > 0
        if rows is not None:
            rows._set(ro)
        if ctx_out is not None:
            ctx_out._set(co)
        self._commit_join(state, state_ctx, spare, tree, ss, sc, t, swapped)
        nch = int(n.value)
        if not own:
            return changed[:nch], None, None, None, swapped
        return changed[:nch], ov[:nch], nv[:nch], fl[:nch], swapped

    def home_block(self):
        """The page-locked result block of join_delta_home / join_delta_home_diffs as a numpy
        view (DG_HOME_DIFFS_WORDS words; the plain call writes a prefix of it)."""
        if getattr(self, "_home", None) is None:
            p = C.c_void_p()
            check(self.lib.dg_host_alloc(self.h, _abi.DG_HOME_DIFFS_WORDS * 8, C.byref(p)))
            self._home = p
        return np.ctypeslib.as_array(C.cast(self._home, C.POINTER(C.c_uint64)),
                                     shape=(_abi.DG_HOME_DIFFS_WORDS,))

    def join_delta_home(self, state: Store, state_ctx: Context, delta: Store, delta_ctx: Context,
                        keys: torch.Tensor, spare: Store, tree: MerkleTree | None = None,
                        _diffs: bool = False):
        """dg_join_delta_home: join_delta for a small delta in one launch chain with one
        host wait, the result (changed keys, their rows, the new context) written into
        page-locked host memory.  Returns None when the library declined (DG_HOME_FALLBACK:
        nothing happened), else (changed keys, rows (key, val, ts, node, cnt), context
        (node, cnt), swapped) as numpy arrays."""
        self._order()
        h = self.home_block()
        ss, sc, sd, cd, sp = state.abi(), state_ctx.abi(), delta.abi(), delta_ctx.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        kp, nk = self._keys(keys)
        sw = C.c_int(0)
        f = self.lib.dg_join_delta_home_diffs if _diffs else self.lib.dg_join_delta_home
        check(f(self.h, C.byref(ss), C.byref(sc), C.byref(sd), C.byref(cd), kp, nk, C.byref(sp), _ref(t),
                self._home, C.byref(sw)))
        return self._home_result(h, state, state_ctx, spare, tree, ss, sc, t, sw)

    def _home_result(self, h, state, state_ctx, spare, tree, ss, sc, t, sw):
        """What join_delta_home and mutate_home return from the result block, and the commit."""
        if int(h[0]) & _abi.DG_HOME_FALLBACK:
            return None
        nch, nr, nc = int(h[1]), int(h[2]), int(h[3])
        S, R0 = _abi.DG_HOME_STRIDE, _abi.DG_HOME_ROWS
        keys_out = h[_abi.DG_HOME_KEYS:_abi.DG_HOME_KEYS + nch].copy()
        rows = (h[R0:R0 + nr].copy(), h[R0 + S:R0 + S + nr].copy(),
                h[R0 + 2 * S:R0 + 2 * S + nr].copy().view(np.int64),
                h[R0 + 4 * S:R0 + 5 * S].view(np.uint32)[:nr].copy(), h[R0 + 3 * S:R0 + 3 * S + nr].copy())
        C0 = _abi.DG_HOME_CTX
        ctx = (h[C0 + _abi.DG_HOME_NODES:C0 + 2 * _abi.DG_HOME_NODES].view(np.uint32)[:nc].copy(),
               h[C0:C0 + nc].copy())
        self._commit_join(state, state_ctx, spare, tree, ss, sc, t, sw.value)
        return keys_out, rows, ctx, bool(sw.value)

    def join_delta_home_diffs(self, state: Store, state_ctx: Context, delta: Store, delta_ctx: Context,
                              keys: torch.Tensor, spare: Store, tree: MerkleTree | None = None):
        """dg_join_delta_home_diffs: join_delta_home plus, for every changed key, its LWW read
        before and after the join out of the same launch and wait (what on_diffs compares).
        None when the library declined, else join_delta_home's tuple followed by (old_val,
        new_val, flags): value ids (0 where the flag is clear) and DG_DIFF_OLD | DG_DIFF_NEW
        bits, entry i describing changed key i."""
        return self._home_diffs(self.join_delta_home(state, state_ctx, delta, delta_ctx, keys, spare, tree,
                                                     _diffs=True))

    def _home_diffs(self, r):
        if r is None:
            return None
        h, n = self.home_block(), len(r[0])
        fl = h[_abi.DG_HOME_DIFF_FLAGS:_abi.DG_HOME_DIFFS_WORDS].view(np.uint8)[:n].copy()
        return r + ((h[_abi.DG_HOME_DIFF_OLD:_abi.DG_HOME_DIFF_OLD + n].copy(),
                     h[_abi.DG_HOME_DIFF_NEW:_abi.DG_HOME_DIFF_NEW + n].copy(), fl),)

    def mutate_home(self, state: Store, ctx: Context, node: int, kind: torch.Tensor, key: torch.Tensor,
                    val: torch.Tensor, ts: torch.Tensor, add_rank: torch.Tensor, n_adds: int, spare: Store,
                    tree: MerkleTree | None = None, _diffs: bool = False):
        """dg_mutate_home: mutate_batch's ops (the same arrays) applied to the resident state in
        one launch and one wait -- mutate_batch followed by join_delta_home with the touched
        keys, without the delta or its dot list ever being made.  Returns what join_delta_home
        returns; None when the library declined (nothing happened: run the two calls)."""
        self._order()
        h = self.home_block()
        m = int(key.numel())
        ss, sc, sp = state.abi(), ctx.abi(), spare.abi()
        t = tree.abi() if tree is not None else None
        sw = C.c_int(0)
        f = self.lib.dg_mutate_home_diffs if _diffs else self.lib.dg_mutate_home
        check(f(self.h, C.byref(ss), C.byref(sc), node, m, _ptr(kind, C.c_void_p) if m else None,
                _ptr(key, _abi.P64), _ptr(val, _abi.P64), _ptr(ts, _abi.PI64), _ptr(add_rank, _abi.P64), n_adds,
                C.byref(sp), _ref(t), self._home, C.byref(sw)))
        return self._home_result(h, state, ctx, spare, tree, ss, sc, t, sw)

    def mutate_home_diffs(self, state: Store, ctx: Context, node: int, kind: torch.Tensor, key: torch.Tensor,
                          val: torch.Tensor, ts: torch.Tensor, add_rank: torch.Tensor, n_adds: int,
                          spare: Store, tree: MerkleTree | None = None):
        """dg_mutate_home_diffs: mutate_home with join_delta_home_diffs' (old_val, new_val, flags)."""
        return self._home_diffs(self.mutate_home(state, ctx, node, kind, key, val, ts, add_rank, n_adds, spare,
                                                 tree, _diffs=True))

    def merkle_update(self, tree: MerkleTree, new: Store, keys: torch.Tensor) -> MerkleTree:
        """MerkleMap.put/delete of the changed `keys` + update_hashes: `tree` indexed
        tree.store; afterwards it indexes `new` (causal_crdt.ex:383-394)."""
        self._order()
        t = tree.abi()
        so, sn = tree.store.abi(), new.abi()
        kp, nk = self._keys(keys)
        check(self.lib.dg_merkle_update(self.h, C.byref(t), C.byref(so), C.byref(sn), kp, nk))
        tree.n_keys = int(t.n_keys) & ((1 << 64) - 1)
        tree.store = new
        return tree

    def merkle_diff(self, a: MerkleTree, b: MerkleTree, cap: int | None = None,
                    with_total: bool = False):
        """The differing keys of the two indexed stores, ascending; with `cap` only the
        first cap (Enum.take(keys, max_sync_size)).  with_total: (keys, total)."""
        self._order()
        if cap is None:
            cap = a.n_keys + b.n_keys
        cap = int(cap)
        # the kernels write into an engine-held buffer of `cap` keys (a fresh cap-sized
        # tensor per call -- 200 MB at config 4 -- cost ~100 us of allocation); the caller
        # gets its own copy of the n keys.  (The next engine call orders itself after the
        # copy: _order.)
        out = getattr(self, "_diff_out", None)
        if out is None or out.numel() < max(cap, 1):
            out = self._diff_out = torch.empty(max(cap, 1), dtype=_I64, device=self.device)
        n, tot = C.c_uint64(), C.c_uint64()
        ta, tb, sa, sb = a.abi(), b.abi(), a.store.abi(), b.store.abi()
        check(self.lib.dg_merkle_diff(self.h, C.byref(ta), C.byref(sa), C.byref(tb), C.byref(sb),
                                      _ptr(out, _abi.P64), cap, C.byref(n), C.byref(tot)))
        keys = out[: n.value].clone()
        return (keys, int(tot.value)) if with_total else keys

    def merkle_diff_take(self, a: MerkleTree, b: MerkleTree, side: int = 1, cap: int | None = None,
                         rows: Store | None = None):
        """dg_merkle_diff_take: merkle_diff(a, b, cap) answered with the kept keys' rows in
        a's store (side 0) or b's (side 1), in one call.  Returns (keys, rows, offs, total):
        rows offs[i]..offs[i + 1] of `rows` are keys[i]'s (offs has len(keys) + 1 entries),
        bit-identical to take_keys(store, keys); total is the untruncated key count.  `rows`
        is sized here when not given, and a DG_E_CAPACITY is retried once with the size the
        call asked for."""
        self._order()
        if cap is None:
            cap = a.n_keys + b.n_keys
        cap = int(cap)
        out = getattr(self, "_diff_out", None)
        if out is None or out.numel() < max(cap, 1):
            out = self._diff_out = torch.empty(max(cap, 1), dtype=_I64, device=self.device)
        offs = torch.empty(cap + 1, dtype=_I64, device=self.device)
        store = b.store if side else a.store
        if rows is None:
            # a sync delta holds a few rows per key (take_keys sizes its output the same way)
            rows = Store.empty(min(max(store.n, 1), max(4 * cap, 256)), self.device)
        n, tot = C.c_uint64(), C.c_uint64()
        ta, tb, sa, sb = a.abi(), b.abi(), a.store.abi(), b.store.abi()

        def call(r):
            so = r.abi()
            rc = self.lib.dg_merkle_diff_take(self.h, C.byref(ta), C.byref(sa), C.byref(tb), C.byref(sb),
                                              int(side), _ptr(out, _abi.P64), cap, _ptr(offs, _abi.P64),
                                              C.byref(so), C.byref(n), C.byref(tot))
            return rc, so

        rc, so = call(rows)
        if rc == _abi.DG_E_CAPACITY and int(so.n) > rows.cap:
            rows = Store.empty(int(so.n), self.device)
            rc, so = call(rows)
        check(rc)
        rows._set(so)
        return out[: n.value].clone(), rows, offs[: n.value + 1], int(tot.value)

    def prepare_merkle_diff(self, a: MerkleTree, b: MerkleTree, out: torch.Tensor, cap: int,
                            d_total: torch.Tensor):
        """Pre-marshal dg_merkle_diff_async for repeated launches (benchmark loops, a
        replica's anti-entropy timer): returns a zero-argument callable that enqueues the
        diff; the first min(total, cap) keys land in `out`, the total in d_total[0]."""
        ta, tb, sa, sb = a.abi(), b.abi(), a.store.abi(), b.store.abi()
        refs = [C.byref(x) for x in (ta, sa, tb, sb)]
        op, dp, f, h = _ptr(out, _abi.P64), _ptr(d_total, _abi.P64), self.lib.dg_merkle_diff_async, self.h

        def launch():
            check(f(h, refs[0], refs[1], refs[2], refs[3], op, int(cap), dp))

        launch._keep = (a, b, out, d_total, ta, tb, sa, sb)
        return launch

    def merkle_prepare(self, tree: MerkleTree, levels: int = 8) -> MerkleCont:
        """MerkleMap.prepare_partial_diff(mm, levels) (causal_crdt.ex:255)."""
        self._order()
        L = min(levels, tree.depth)
        cont = MerkleCont.empty(1 << L, 1, self.device)
        c = cont.abi()
        check(self.lib.dg_merkle_prepare(self.h, C.byref(tree.abi()), levels, C.byref(c)))
        cont._set(c)
        return cont

    @staticmethod
    def _cont_sizes(cont: MerkleCont, max_entries):
        """The (entries, buckets) a hop's output continuation is first given."""
        oc, ob = 4 * max(cont.n, 1), max(cont.n, 1)
        if max_entries is not None:
            oc = min(oc, max(int(max_entries), 1))
        return oc, ob

    def _hop(self, home, tree, cont, levels, max_entries, cap):
        """The body of merkle_continue and (home) merkle_continue_home: the call, run again
        with the output continuation grown to the sizes a DG_E_CAPACITY answer reports."""
        self._order()
        s = tree.store
        if cap is None:
            cap = max(cont.n, 1) + s.n
        keys = torch.empty(max(int(cap), 1), dtype=_I64, device=self.device)
        cin = cont.abi()
        t, ss = tree.abi(), s.abi()
        mx = (1 << 64) - 1 if max_entries is None else int(max_entries)
        f, extra = (self.lib.dg_merkle_continue_home, (mx,)) if home else (self.lib.dg_merkle_continue, ())
        out_cap, out_bcap = self._cont_sizes(cont, max_entries)
        for _ in range(3):  # grow the output continuation to the sizes the call reports
            out = MerkleCont.empty(out_cap, out_bcap, self.device)
            co = out.abi()
            nk, tot, st = C.c_uint64(), C.c_uint64(), C.c_int()
            rc = f(self.h, C.byref(t), C.byref(ss), C.byref(cin), levels, *extra, C.byref(co),
                   _ptr(keys, _abi.P64), int(cap), C.byref(nk), C.byref(tot), C.byref(st))
            if rc != _abi.DG_E_CAPACITY:
                break
            out_cap, out_bcap = max(int(co.n), out_cap), max(int(co.n_buckets), out_bcap)
        check(rc)
        if home and st.value == _abi.DG_CONT_DECLINED:
            return ("declined",)
        if st.value == 1:
            out._set(co)
            return ("continue", out)
        return ("ok", keys[: nk.value], int(tot.value))

    def merkle_continue(self, tree: MerkleTree, cont: MerkleCont, levels: int = 8,
                        cap: int | None = None):
        """MerkleMap.continue_partial_diff(cont, mm, levels) (causal_crdt.ex:96) on this
        replica's tree: ("continue", MerkleCont) or ("ok", keys, total)."""
        return self._hop(False, tree, cont, levels, None, cap)

    def merkle_continue_home(self, tree: MerkleTree, cont: MerkleCont, levels: int = 8,
                             max_entries: int | None = None, cap: int | None = None):
        """dg_merkle_continue_home: one hop (continue_partial_diff + truncate_diff to
        max_entries; None: :infinite) in one launch with one host wait.  ("continue",
        MerkleCont), ("ok", keys, total), or ("declined",) for a continuation over the
        one-workgroup limits (then merkle_continue)."""
        return self._hop(True, tree, cont, levels, max_entries, cap)

    def merkle_continues(self, tree: MerkleTree, conts, levels: int = 8, max_entries: int | None = None,
                         caps=None, retry: bool = True):
        """dg_merkle_continues: the hops of k <= 64 pending continuations (k neighbours'
        messages) against ONE tree in one launch with one host wait.  A list whose element j is
        what merkle_continue_home(tree, conts[j], levels, max_entries) returns, or ("error", code)
        where that call would raise (one hop's error leaves the others' results).  `caps`: per hop the (entries, buckets)
        its output is first given (default: merkle_continue_home's); a hop that reports
        DG_E_CAPACITY is retried, alone with the other such hops, at the sizes it reported
        (retry=False: its element is ("capacity", entries, buckets), the sizes needed)."""
        return self._hops(tree, conts, None, levels, max_entries, caps, None, retry)

    def merkle_continues_take(self, tree: MerkleTree, conts, want_rows, levels: int = 8,
                              max_entries: int | None = None, caps=None, row_caps=None, retry: bool = True):
        """dg_merkle_continues_take: merkle_continues whose {:ok, keys} hops with want_rows[j] set
        also return Map.take(value, keys) of the keys they keep, out of the same launch and wait.
        Such a hop keeps the first max_entries keys (truncate(keys, max_sync_size); None: all)
        and its element is ("ok", keys, total, offs, Store): rows [offs[i], offs[i + 1]) of the
        Store are keys[i]'s, what take_keys(tree.store, keys) returns.  Every other element is
        merkle_continues'.  `row_caps`: per hop the rows its Store is first given (default:
        take_keys'); a take that reports DG_E_CAPACITY is retried at the size it reported
        (retry=False: ("ok", keys, total, None, ("capacity", rows needed)))."""
        return self._hops(tree, conts, want_rows, levels, max_entries, caps, row_caps, retry)

    def _hops(self, tree, conts, want_rows, levels, max_entries, caps, row_caps, retry):
        """The body of merkle_continues (want_rows None) and merkle_continues_take: the hops'
        buffers, up to three launches -- each of the hops (and takes) that reported
        DG_E_CAPACITY in the one before, at the sizes they reported -- and every hop's result."""
        self._order()
        conts = list(conts)
        k = len(conts)
        take = want_rows is not None
        want = [bool(w) for w in want_rows] if take else [False] * k
        assert len(want) == k
        s = tree.store
        mx = (1 << 64) - 1 if max_entries is None else int(max_entries)
        t, ss = tree.abi(), s.abi()
        hops = (_abi.dg_cont_hop * max(k, 1))()
        cins = [c.abi() for c in conts]
        sizes, outs, cos, keys = [], [None] * k, [None] * k, []
        rsize, rows, offs, takes = [0] * k, [None] * k, [None] * k, [None] * k
        for j, c in enumerate(conts):
            sizes.append(tuple(caps[j]) if caps is not None and caps[j] is not None
                         else self._cont_sizes(c, max_entries))
            cap = max(c.n, 1) + s.n
            if want[j] and max_entries is not None:
                cap = min(cap, max(int(max_entries), 1))
            keys.append(torch.empty(max(int(cap), 1), dtype=_I64, device=self.device))
            hops[j].in_ = C.pointer(cins[j])
            hops[j].keys = keys[j].data_ptr()
            hops[j].cap = int(cap)
            if want[j]:
                # take_keys' rule: room for four rows per key, the store's rows at the most
                rsize[j] = (int(row_caps[j]) if row_caps is not None and row_caps[j] is not None
                            else min(max(s.n, 1), max(4 * int(cap), 256)))
                offs[j] = torch.empty(int(cap) + 1, dtype=_I64, device=self.device)
        todo = list(range(k))
        res = [None] * k
        for attempt in range(3):
            batch = (_abi.dg_cont_hop * max(len(todo), 1))()
            tptr = (C.POINTER(_abi.dg_cont_take) * max(len(todo), 1))() if take else None
            for i, j in enumerate(todo):
                outs[j] = MerkleCont.empty(sizes[j][0], sizes[j][1], self.device)
                cos[j] = outs[j].abi()
                hops[j].out = C.pointer(cos[j])
                batch[i] = hops[j]
                if want[j]:
                    rows[j] = Store.empty(max(rsize[j], 1), self.device)
                    takes[j] = _abi.dg_cont_take(rows=rows[j].abi(), offs=offs[j].data_ptr())
                    takes[j].rows.cap = rsize[j]
                    tptr[i] = C.pointer(takes[j])
            if take:
                check(self.lib.dg_merkle_continues_take(self.h, C.byref(t), C.byref(ss), len(todo), batch, tptr,
                                                        levels, mx))
            else:
                check(self.lib.dg_merkle_continues(self.h, C.byref(t), C.byref(ss), len(todo), batch, levels, mx))
            again = []
            for i, j in enumerate(todo):
                h = batch[i]
                if h.rc == _abi.DG_E_CAPACITY and not retry:
                    res[j] = ("capacity", int(cos[j].n), int(cos[j].n_buckets))
                elif h.rc == _abi.DG_E_CAPACITY and attempt < 2:
                    sizes[j] = (max(int(cos[j].n), sizes[j][0]), max(int(cos[j].n_buckets), sizes[j][1]))
                    again.append(j)
                elif h.rc != _abi.DG_OK:
                    res[j] = ("error", h.rc)
                elif h.status == _abi.DG_CONT_DECLINED:
                    res[j] = ("declined",)
                elif h.status == 1:
                    outs[j]._set(cos[j])
                    res[j] = ("continue", outs[j])
                elif not want[j] or h.n_keys == 0:  # ({:ok, []} took no rows)
                    res[j] = ("ok", keys[j][: h.n_keys], int(h.n_total))
                elif takes[j].rc == _abi.DG_E_CAPACITY and retry and attempt < 2:
                    rsize[j] = int(takes[j].rows.n)
                    again.append(j)
                elif takes[j].rc == _abi.DG_E_CAPACITY:
                    res[j] = ("ok", keys[j][: h.n_keys], int(h.n_total), None, ("capacity", int(takes[j].rows.n)))
                else:
                    check(takes[j].rc)
                    rows[j]._set(takes[j].rows)
                    res[j] = ("ok", keys[j][: h.n_keys], int(h.n_total), offs[j][: h.n_keys + 1], rows[j])
            todo = again
            if not todo:
                break
        return res

    def merkle_truncate(self, tree: MerkleTree, cont: MerkleCont, max_entries: int) -> MerkleCont:
        """MerkleMap.truncate_diff(cont, max_sync_size) (causal_crdt.ex:98,212-214)."""
        c = cont.abi()
        check(self.lib.dg_merkle_truncate(self.h, C.byref(tree.abi()), C.byref(c), int(max_entries)))
        cont._set(c)
        return cont

    # ---------------------------------------------------------------- marshalling
    def sort_store(self, s: Store, out: Store | None = None) -> Store:
        """dg_sort_store: rows in any order (e.g. a map walk) -> sorted by (key, val, ts,
        node, cnt), duplicates dropped."""
        self._order()
        if out is None:
            out = Store.empty(max(s.n, 1), self.device)
        si, so = s.abi(), out.abi()
        check(self.lib.dg_sort_store(self.h, C.byref(si), C.byref(so)))
        out._set(so)
        return out

    def sort_context(self, c: Context, out: Context | None = None) -> Context:
        """dg_sort_context: a VV by node, a dot set by (node, cnt)."""
        self._order()
        if out is None:
            out = Context.empty(c.kind, max(c.n, 1), self.device)
        ci, co = c.abi(), out.abi()
        check(self.lib.dg_sort_context(self.h, C.byref(ci), C.byref(co)))
        out._set(co)
        return out

    # ---------------------------------------------------------------- interning
    def remap_values(self, s: Store, old_ids: np.ndarray, new_ids: np.ndarray):
        """Rewrite s.val in place after a value relabel (dg_remap_values): old_ids /
        new_ids ascending uint64, the monotone map the Universe produced."""
        self._order()
        o = _np_to_dev(np.asarray(old_ids, np.uint64), np.int64, self.device)
        w = _np_to_dev(np.asarray(new_ids, np.uint64), np.int64, self.device)
        ss = s.abi()
        check(self.lib.dg_remap_values(self.h, C.byref(ss), _ptr(o, _abi.P64), _ptr(w, _abi.P64),
                                       int(len(old_ids))))

    def mark_ids(self, stores, column: int, ids):
        """dg_mark_ids: which of `ids` (strictly ascending u64 ids: a numpy array, or a device
        int64 tensor holding their bits) occur in `column` (_abi.DG_COL_KEY / DG_COL_VAL) of
        some row of `stores`.  Returns (used, n_used, n_unknown): a device uint8 tensor of
        len(ids) flags, the number of ones, and the number of rows whose id is not in `ids`
        (canonical integer values not counted on the value column)."""
        self._order()
        if not isinstance(ids, torch.Tensor):
            a = np.ascontiguousarray(np.asarray(ids, np.uint64))
            ids = (_np_to_dev(a, np.int64, self.device) if len(a)
                   else torch.zeros(0, dtype=_I64, device=self.device))
        n = int(ids.numel())
        used = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        k = len(stores)
        arr = self._structs(stores, _abi.dg_store)
        nu, nx = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.dg_mark_ids(self.h, arr, k, int(column), _ptr(ids, _abi.P64), n,
                                   C.c_void_p(used.data_ptr()), C.byref(nu), C.byref(nx)))
        return used[:n], int(nu.value), int(nx.value)

    def store_check(self, s: Store):
        self._order()
        ss = s.abi()
        check(self.lib.dg_store_check(self.h, C.byref(ss)))


def u64(t: torch.Tensor) -> np.ndarray:
    """Device int64 tensor holding u64 bits -> numpy uint64."""
    return t.cpu().numpy().view(np.uint64)


__all__ = ["Store", "Context", "MerkleTree", "MerkleCont", "TermHashes", "Engine", "fold_roots", "u64",
           "DG_CTX_VV", "DG_CTX_DOTS"]
