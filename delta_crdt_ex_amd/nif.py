"""Python mirror of the Erlang NIF `DeltaCrdt.GPU` (c_src/deltagpu_nif.c).

The NIF is a term layer over c_src/replica.c (the device-resident replica state with
versions, replica.h); this module is the same term layer over the SAME compiled code
(c_src/_build/libdgreplica.so, ctypes), function for function and with the NIF's return
shapes, so the Elixir dispatch of INTEGRATION.md §3 can be exercised without a BEAM
(tests/binding_mirror.py, tests/test_gpu_binding.py):

    engine_open(device)                             -> ("ok", engine)
    state_load(engine, dots, value)                 -> ("ok", state, version)
    join_delta(state, version, dots, value, keys)   -> ("ok", version', new_dots, changed)
    mutate_batch(state, version, node, ops)         -> ("ok", version', new_dots, changed)
    join_delta_diffs(state, version, dots, value, keys)
    mutate_batch_diffs(state, version, node, ops)   -> ("ok", version', new_dots, changed, diffs)
    join_deltas(state, version, [(dots, value, keys), ...])
                                                    -> ("ok", version', new_dots, changed)
    join_deltas_diffs(state, version, [(dots, value, keys), ...])
                                                    -> ("ok", version', new_dots, changed, diffs)
    read(state, version, keys | "all")              -> ("ok", {key: value})
    take(state, version, keys)                      -> ("ok", value_map)
    take_batch(state, version, [keys, ...])         -> ("ok", [value_map, ...])
    merkle_build(state, version, depth)             -> "ok"
    merkle_prepare(state, version, levels)          -> ("continue", bytes)
    merkle_continue(state, version, cont, levels, max_sync_size | "infinite")
                                                    -> ("continue", bytes) | ("ok", keys)
    merkle_continue_batch(state, version, [cont, ...], levels, max_sync_size | "infinite")
                                                    -> ("ok", [("continue", bytes) | ("ok", keys), ...])
    merkle_continue_take_batch(state, version, [cont, ...], [want, ...], levels, max_sync_size | "infinite")
                                                    -> ("ok", [("continue", bytes) | ("ok", keys)
                                                               | ("ok", keys, value_map), ...])
    sweep(engine)                                   -> ("ok", {"values": (before, after),
                                                               "keys": (before, after)})
    resolve_keys(engine, keys)                      -> keys
    errors: ("error", "stale") for a version that is not the state's (an older struct),
            ("error", (code, message)) otherwise.

Terms are the package's stand-ins (delta_crdt_ex_amd/terms.py): a MapSet of dots is a
frozenset of (node, counter), a compressed context a {node: max} dict, a value map
{key: {(value, ts): frozenset(dots)}}, nil None.  An engine may be opened with `wrap` /
`unwrap` functions applied to every term crossing it (the tests keep their terms in an
exact-equality form, as BEAM maps compare keys, and pass the conversions).

`diffs` is what on_diffs receives (diffs_to_callback/3, causal_crdt.ex:361-381), computed
from the device's reads of the changed keys before and after the join -- no old struct is
read: [("add", key, value) | ("remove", key)] in ascending key-id order, the order of
`changed`.  The reference emits them in the order of its `keys` argument; a consumer must
not rely on the order inside one callback list.

Interning is the NIF's (c_src/marshal.c), mirrored by interning.Universe with the same
ids: key ids are hashes, value ids order-preserving, node ids dense; a relabel rewrites
every live state of the engine (dgr_remap).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi, interning
from ._abi import DG_CTX_DOTS, DG_CTX_VV, dg_context, dg_store
from .terms import Atom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "c_src", "_build", "libdgreplica.so")

DGR_E_STALE = -16
U64_MAX = (1 << 64) - 1


class dgr_diffs(C.Structure):
    _fields_ = [("n", C.c_uint64), ("old_val", C.c_void_p), ("new_val", C.c_void_p),
                ("flags", C.c_void_p)]


class dgr_changed(C.Structure):
    _fields_ = [("version", C.c_uint64), ("n_changed", C.c_uint64), ("keys", C.c_void_p),
                ("rows", dg_store), ("ctx", dg_context)]


class dgr_hop_rows(C.Structure):
    _fields_ = [("rows", dg_store), ("offs", C.c_void_p)]


class dgr_taken(C.Structure):
    _fields_ = [("n_keys", C.c_uint64), ("keys", C.c_void_p), ("masks", C.c_void_p), ("offs", C.c_void_p),
                ("rows", dg_store)]


class dgr_cont_result(C.Structure):
    _fields_ = [("rc", C.c_int), ("status", C.c_int), ("bin", C.c_void_p), ("len", C.c_uint64),
                ("keys", C.c_void_p), ("n_keys", C.c_uint64)]


VP, U64, I32 = C.c_void_p, C.c_uint64, C.c_int
PU64 = C.POINTER(C.c_uint64)
_SIGS = {
    "dgr_engine_open": (I32, [I32, C.POINTER(VP)]),
    "dgr_engine_close": (I32, [VP]),
    "dgr_live_states": (U64, [VP]),
    "dgr_deltas_route_stats": (I32, [VP, PU64]),
    "dgr_mutate_route_stats": (I32, [VP, PU64]),
    "dgr_dg": (VP, [VP]),
    "dgr_refresh_terms": (I32, [VP, VP, U64, VP, VP, U64]),
    "dgr_remap": (I32, [VP, VP, VP, U64]),
    "dgr_sweep": (I32, [VP, I32, VP, U64, C.POINTER(VP), PU64, PU64]),
    "dgr_state_load": (I32, [VP, C.POINTER(dg_store), C.POINTER(dg_context), C.POINTER(VP)]),
    "dgr_state_free": (I32, [VP]),
    "dgr_state_version": (U64, [VP]),
    "dgr_state_rows": (U64, [VP]),
    "dgr_state_has_tree": (I32, [VP]),
    "dgr_join_delta": (I32, [VP, U64, C.POINTER(dg_store), C.POINTER(dg_context), VP, U64,
                             C.POINTER(dgr_changed)]),
    "dgr_mutate_batch": (I32, [VP, U64, C.c_uint32, U64, VP, VP, VP, VP, C.POINTER(dgr_changed)]),
    "dgr_join_delta_diffs": (I32, [VP, U64, C.POINTER(dg_store), C.POINTER(dg_context), VP, U64,
                                   C.POINTER(dgr_changed), C.POINTER(dgr_diffs)]),
    "dgr_mutate_batch_diffs": (I32, [VP, U64, C.c_uint32, U64, VP, VP, VP, VP, C.POINTER(dgr_changed),
                                     C.POINTER(dgr_diffs)]),
    "dgr_sync_from": (I32, [VP, U64, VP, U64, U64, C.POINTER(dgr_changed), PU64]),
    "dgr_sync_from_diffs": (I32, [VP, U64, VP, U64, U64, C.POINTER(dgr_changed), C.POINTER(dgr_diffs), PU64]),
    "dgr_join_deltas": (I32, [VP, U64, I32, C.POINTER(dg_store), C.POINTER(dg_context), C.POINTER(VP), PU64,
                              C.POINTER(dgr_changed)]),
    "dgr_join_deltas_diffs": (I32, [VP, U64, I32, C.POINTER(dg_store), C.POINTER(dg_context), C.POINTER(VP),
                                    PU64, C.POINTER(dgr_changed), C.POINTER(dgr_diffs)]),
    # (the batch's packing alone, host code: c_src/test_batch.c checks it)
    "dgr_batch_words": (U64, [I32, C.POINTER(dg_store), C.POINTER(dg_context), PU64]),
    "dgr_batch_pack": (U64, [VP, VP, I32, C.POINTER(dg_store), C.POINTER(dg_context), C.POINTER(VP), PU64,
                             C.POINTER(dg_store), C.POINTER(dg_context), C.POINTER(VP), PU64]),
    "dgr_read": (I32, [VP, U64, I32, VP, U64, C.POINTER(VP), C.POINTER(VP), PU64]),
    "dgr_take": (I32, [VP, U64, VP, U64, C.POINTER(dg_store)]),
    "dgr_take_batch": (I32, [VP, U64, I32, C.POINTER(VP), PU64, C.POINTER(dgr_taken)]),
    # (its packing alone, host code: c_src/test_takes.c checks it)
    "dgr_mutate_words": (U64, [U64]),
    "dgr_mutate_pack": (I32, [PU64, U64, VP, PU64, PU64, VP, PU64]),
    "dgr_takes_words": (U64, [I32, PU64]),
    "dgr_takes_pack": (U64, [VP, VP, I32, C.POINTER(VP), PU64, C.POINTER(VP), PU64]),
    "dgr_merkle_build": (I32, [VP, U64, C.c_uint32]),
    "dgr_merkle_prepare": (I32, [VP, U64, C.c_uint32, C.POINTER(VP), PU64]),
    "dgr_merkle_continue": (I32, [VP, U64, C.c_char_p, U64, C.c_uint32, U64, C.POINTER(I32),
                                  C.POINTER(VP), PU64, C.POINTER(VP), PU64]),
    "dgr_merkle_continue_batch": (I32, [VP, U64, I32, C.POINTER(C.c_char_p), PU64, C.c_uint32, U64,
                                        C.POINTER(dgr_cont_result)]),
    "dgr_merkle_continue_take_batch": (I32, [VP, U64, I32, C.POINTER(C.c_char_p), PU64, C.c_char_p, C.c_uint32,
                                             U64, C.POINTER(dgr_cont_result), C.POINTER(dgr_hop_rows)]),
}

_lib = None


def load():
    """libdgreplica.so over the in-tree libdeltagpu.so (raises if either is missing or
    stale: there is no fallback)."""
    global _lib
    if _lib is None:
        _abi.load()  # the digest check of the library libdgreplica links
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C c_src`")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib


def _err(rc):
    if rc == DGR_E_STALE:
        return ("error", "stale")
    msg = (_abi.load().dg_last_error() or b"").decode(errors="replace")
    return ("error", (rc, msg))


def _ident(t):
    return t


class Engine:
    """`engine` resource: a dgr_engine (one dg_engine, one HIP stream) and the interning
    universe of this "BEAM node"."""

    def __init__(self, device: int = 0, wrap=None, unwrap=None):
        self.lib = load()
        self.ptr = VP()
        rc = self.lib.dgr_engine_open(device, C.byref(self.ptr))
        if rc:
            raise _abi.DeltaGpuError(rc, "dgr_engine_open failed")
        self.universe = interning.Universe()
        self.universe.remap_hook = self._remap
        self.wrap = wrap or _ident
        self.unwrap = unwrap or _ident
        self.states = []

    def _remap(self, old_ids, new_ids):  # remap_live
        old = np.ascontiguousarray(old_ids, np.uint64)
        new = np.ascontiguousarray(new_ids, np.uint64)
        rc = self.lib.dgr_remap(self.ptr, old.ctypes.data, new.ctypes.data, len(old))
        if rc:
            raise _abi.DeltaGpuError(rc, "dgr_remap failed")

    def refresh_terms(self):
        nh, vid, vh = self.universe.term_tables()
        return self.lib.dgr_refresh_terms(self.ptr, nh.ctypes.data, len(nh), vid.ctypes.data,
                                          vh.ctypes.data, len(vid))

    def _mark(self, column: int, ids: np.ndarray):
        """dgr_sweep: the flags of `ids` (ascending) over the rows of every live state"""
        ids = np.ascontiguousarray(ids, np.uint64)
        p, nu, nx = VP(), C.c_uint64(), C.c_uint64()
        rc = self.lib.dgr_sweep(self.ptr, column, ids.ctypes.data, len(ids), C.byref(p), C.byref(nu),
                                C.byref(nx))
        if rc:
            return rc, None, 0
        used = (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(len(ids),)).copy()
                if len(ids) else np.zeros(0, np.uint8))
        return 0, used, int(nx.value)

    def sweep(self, keys: bool = True, keep_values=(), keep_keys=()):
        """Drop the universe's table values (and keys) that no live state of this engine
        names any more (dgr_sweep + Universe.sweep; the NIF's sweep/1 does the same with
        dgm_sweep_values / dgm_sweep_keys).  State versions do not change.  Terms on their
        way into a delta that is not joined yet are pinned with keep_values / keep_keys.
        Returns the NIF's shape: ("ok", {"values": (before, after), "keys": (before, after)})."""
        U = self.universe
        vids, _t = U.value_ids()
        rc, used_v, unknown = self._mark(_abi.DG_COL_VAL, np.array(vids, np.uint64))
        if rc:
            return _err(rc)
        if unknown:
            return ("error", (_abi.DG_E_INVAL, f"{unknown} rows hold a value id the table lacks"))
        used_k = None
        if keys:
            rc, used_k, unknown = self._mark(_abi.DG_COL_KEY, U.key_ids())
            if rc:
                return _err(rc)
            if unknown:
                return ("error", (_abi.DG_E_INVAL, f"{unknown} rows hold a key id the table lacks"))
        return ("ok", U.sweep(used_v, used_k, keep_values=[self.unwrap(t) for t in keep_values],
                              keep_keys=[self.unwrap(t) for t in keep_keys]))

    def deltas_route_stats(self):
        """(tried, served, declined): how often this engine's join_deltas[_diffs] tried
        dg_join_deltas_keyed, was served by it and was declined (dgr_deltas_route_stats; the
        route is DGR_DELTAS_ROUTE at engine open).  Not a NIF function: tests and A/B."""
        out = (C.c_uint64 * 3)()
        rc = self.lib.dgr_deltas_route_stats(self.ptr, out)
        if rc:
            raise _abi.DeltaGpuError(rc, "dgr_deltas_route_stats failed")
        return tuple(int(x) for x in out)

    def mutate_route_stats(self):
        """(tried, served, declined): how often this engine's mutate_batch[_diffs] tried
        dg_mutate_home, was served by it and was declined (dgr_mutate_route_stats; the route is
        DGR_MUTATE_ROUTE at engine open).  Not a NIF function: tests and A/B."""
        out = (C.c_uint64 * 3)()
        rc = self.lib.dgr_mutate_route_stats(self.ptr, out)
        if rc:
            raise _abi.DeltaGpuError(rc, "dgr_mutate_route_stats failed")
        return tuple(int(x) for x in out)

    def close(self):
        for s in self.states:
            s.free()
        self.states = []
        if self.ptr:
            self.lib.dgr_engine_close(self.ptr)
            self.ptr = VP()


class State:
    """`state` resource: one device-resident replica state (dgr_state)."""

    def __init__(self, engine: Engine, ptr):
        self.engine = engine
        self.ptr = ptr

    def free(self):
        if self.ptr:
            self.engine.lib.dgr_state_free(self.ptr)
            self.ptr = None

    @property
    def version(self):
        return int(self.engine.lib.dgr_state_version(self.ptr))

    @property
    def n_rows(self):
        return int(self.engine.lib.dgr_state_rows(self.ptr))


# ------------------------------------------------------------------ marshal
class _Rows:
    """Host rows and a context, as dgm_rows (the columns of a dg_store / dg_context)."""

    def __init__(self):
        self.k, self.v, self.t, self.n, self.c = [], [], [], [], []
        self.kind, self.cn, self.cc = DG_CTX_DOTS, [], []

    def store(self):
        self._a = (np.array(self.k, np.uint64), np.array(self.v, np.uint64),
                   np.array(self.t, np.int64), np.array(self.n, np.uint32),
                   np.array(self.c, np.uint64))
        k, v, t, n, c = self._a
        return dg_store(k.ctypes.data, v.ctypes.data, t.ctypes.data, n.ctypes.data, c.ctypes.data,
                        len(k), len(k))

    def context(self):
        self._c = (np.array(self.cn, np.uint32), np.array(self.cc, np.uint64))
        n, c = self._c
        return dg_context(self.kind, 0, n.ctypes.data, c.ctypes.data, len(n), len(n))


def _marshal_dots(eng: Engine, dots, out: _Rows):
    """a context: a MapSet of dots (DG_CTX_DOTS) or a %{node => max} VV (DG_CTX_VV)"""
    U, un = eng.universe, eng.unwrap
    if isinstance(dots, dict):
        out.kind = DG_CTX_VV
        items = dots.items()
    else:
        out.kind = DG_CTX_DOTS
        items = dots
    for node, cnt in items:
        out.cn.append(U.node(un(node)))
        out.cc.append(int(cnt))


def _marshal_value(eng: Engine, value, out: _Rows):
    """walk %{key => %{{v, ts} => MapSet[{node, counter}]}} in map order into host rows"""
    U, un = eng.universe, eng.unwrap
    for entries in value.values():  # pass 1: values first (a relabel re-spaces ids)
        for (v, _ts) in entries:
            U.value(un(v))
    for key, entries in value.items():
        kid = U.key(un(key))
        for (v, ts), dots in entries.items():
            vid = U.value(un(v))
            for node, cnt in dots:
                out.k.append(kid)
                out.v.append(vid)
                out.t.append(int(ts))
                out.n.append(U.node(un(node)))
                out.c.append(int(cnt))


KEY_TAG = Atom("$dg_key")


def key_placeholder(kid: int):
    """`{:"$dg_key", id}`: a differing key this node never interned (only the peer holds
    it), named by its id.  Every NIF that takes keys accepts it as that id; resolve_keys
    turns it back into the key's term on a node that knows the key."""
    return (KEY_TAG, int(kid))


def _key_id(eng: Engine, k):
    t = eng.unwrap(k)
    if isinstance(t, tuple) and len(t) == 2 and isinstance(t[0], Atom) and t[0] == KEY_TAG:
        return int(t[1])
    return eng.universe.key(t)


def _marshal_keys(eng: Engine, keys):
    return np.array([_key_id(eng, k) for k in keys], np.uint64)


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    ct = {np.uint64: C.c_uint64, np.int64: C.c_int64, np.uint32: C.c_uint32}[dtype]
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).copy()


def _value_term(eng: Engine, vid: int):
    return eng.wrap(eng.universe.value_term(int(vid)))


def _unmarshal_rows(eng: Engine, s: dg_store):
    """host rows (store order) -> {key: {(v, ts): frozenset(dots)}}"""
    n = int(s.n)
    k, v = _arr(s.key, n, np.uint64), _arr(s.val, n, np.uint64)
    t, nd, c = _arr(s.ts, n, np.int64), _arr(s.node, n, np.uint32), _arr(s.cnt, n, np.uint64)
    U, w = eng.universe, eng.wrap
    out: dict = {}
    for i in range(n):
        ent = out.setdefault(w(U.key_term(int(k[i]))), {})
        ent.setdefault((_value_term(eng, v[i]), int(t[i])), set()).add(
            (w(U.node_term(int(nd[i]))), int(c[i])))
    return {key: {e: frozenset(d) for e, d in ents.items()} for key, ents in out.items()}


def _unmarshal_dots(eng: Engine, c: dg_context):
    n = int(c.n)
    node, cnt = _arr(c.node, n, np.uint32), _arr(c.cnt, n, np.uint64)
    U, w = eng.universe, eng.wrap
    if c.kind == DG_CTX_VV:
        return {w(U.node_term(int(a))): int(b) for a, b in zip(node, cnt)}
    return frozenset((w(U.node_term(int(a))), int(b)) for a, b in zip(node, cnt))


def _changed_result(eng: Engine, ch: dgr_changed):
    values = _unmarshal_rows(eng, ch.rows)
    dots = _unmarshal_dots(eng, ch.ctx)
    keys = _arr(ch.keys, int(ch.n_changed), np.uint64)
    changed = []
    for kid in keys:
        k = eng.wrap(eng.universe.key_term(int(kid)))
        changed.append((k, values.get(k)))  # None: the key's entries all went
    return ("ok", int(ch.version), dots, changed)


DIFF_NONE, DIFF_ADD, DIFF_REMOVE = 0, 1, 2


def classify_diffs(old_val, new_val, flags, nil_id):
    """marshal.h dgm_classify_diffs: diffs_to_callback/3's case (causal_crdt.ex:368-374)
    over value ids -- per entry DIFF_NONE, DIFF_ADD or DIFF_REMOVE.  A side is absent when
    its flag is clear or its id is nil's (`nil_id`, None when nil was never interned)."""
    kind = []
    for o, n, f in zip(old_val, new_val, flags):
        has_o = bool(int(f) & _abi.DG_DIFF_OLD) and not (nil_id is not None and int(o) == nil_id)
        has_n = bool(int(f) & _abi.DG_DIFF_NEW) and not (nil_id is not None and int(n) == nil_id)
        if not has_n:
            kind.append(DIFF_REMOVE if has_o else DIFF_NONE)
        else:
            kind.append(DIFF_NONE if has_o and int(o) == int(n) else DIFF_ADD)
    return kind


def _diffs_result(eng: Engine, ch: dgr_changed, df: dgr_diffs):
    res = _changed_result(eng, ch)
    n = int(df.n)
    keys = _arr(ch.keys, n, np.uint64)
    ov, nv = _arr(df.old_val, n, np.uint64), _arr(df.new_val, n, np.uint64)
    fl = (np.ctypeslib.as_array(C.cast(df.flags, C.POINTER(C.c_uint8)), shape=(n,)).copy()
          if n else np.zeros(0, np.uint8))
    U, w = eng.universe, eng.wrap
    diffs = []
    for kid, v, kind in zip(keys, nv, classify_diffs(ov, nv, fl, U.value_find(None))):
        if kind == DIFF_ADD:
            diffs.append(("add", w(U.key_term(int(kid))), _value_term(eng, v)))
        elif kind == DIFF_REMOVE:
            diffs.append(("remove", w(U.key_term(int(kid)))))
    return res + (diffs,)


# ------------------------------------------------------------------ the NIFs
def engine_open(device: int = 0, wrap=None, unwrap=None):
    return ("ok", Engine(device, wrap, unwrap))


def state_load(engine: Engine, dots, value):
    h = _Rows()
    _marshal_dots(engine, dots, h)
    _marshal_value(engine, value, h)
    st, cx = h.store(), h.context()
    ptr = VP()
    rc = engine.lib.dgr_state_load(engine.ptr, C.byref(st), C.byref(cx), C.byref(ptr))
    if rc:
        return _err(rc)
    s = State(engine, ptr)
    engine.states.append(s)
    return ("ok", s, s.version)


def join_delta(state: State, version: int, dots, value, keys, _diffs: bool = False):
    eng = state.engine
    h = _Rows()
    _marshal_dots(eng, dots, h)
    _marshal_value(eng, value, h)
    kid = _marshal_keys(eng, keys)
    if eng.lib.dgr_state_has_tree(state.ptr):
        rc = eng.refresh_terms()
        if rc:
            return _err(rc)
    st, cx = h.store(), h.context()
    ch = dgr_changed()
    if _diffs:
        df = dgr_diffs()
        rc = eng.lib.dgr_join_delta_diffs(state.ptr, version, C.byref(st), C.byref(cx), kid.ctypes.data,
                                          len(kid), C.byref(ch), C.byref(df))
        return _err(rc) if rc else _diffs_result(eng, ch, df)
    rc = eng.lib.dgr_join_delta(state.ptr, version, C.byref(st), C.byref(cx), kid.ctypes.data,
                                len(kid), C.byref(ch))
    if rc:
        return _err(rc)
    return _changed_result(eng, ch)


def join_delta_diffs(state: State, version: int, dots, value, keys):
    """join_delta that also returns on_diffs' list, from the device's reads of the changed
    keys before and after the join (dgr_join_delta_diffs): no old struct is read."""
    return join_delta(state, version, dots, value, keys, _diffs=True)


def sync_from(dst: State, dst_version: int, src: State, src_version: int, max_sync_size="infinite",
              _diffs: bool = False):
    """sync_from(dst, dst_version, src, src_version, max_sync_size | :infinite) -> {:ok, version',
    new_dots, changed, n_total}: one anti-entropy exchange from `src` toward `dst`, two replicas
    attached to one engine, device to device (dgr_sync_from): the trees' diff, src's rows of the
    first max_sync_size differing keys and their join into dst, with no row turned into a term.
    n_total is the untruncated number of differing keys; run another round while it exceeds
    max_sync_size.  Marshals exactly as join_delta does."""
    if not isinstance(dst, State) or not isinstance(src, State):
        return _err(_abi.DG_E_INVAL)
    eng = dst.engine
    if max_sync_size in ("infinite", None):
        ms = 0
    elif isinstance(max_sync_size, int) and max_sync_size > 0:
        ms = max_sync_size
    else:
        return _err(_abi.DG_E_INVAL)
    if eng.lib.dgr_state_has_tree(dst.ptr) and eng.lib.dgr_state_has_tree(src.ptr) and src.engine is eng:
        rc = eng.refresh_terms()
        if rc:
            return _err(rc)
    ch, tot = dgr_changed(), C.c_uint64()
    if _diffs:
        df = dgr_diffs()
        rc = eng.lib.dgr_sync_from_diffs(dst.ptr, dst_version, src.ptr, src_version, ms, C.byref(ch), C.byref(df),
                                         C.byref(tot))
        if rc:
            return _err(rc)
        res = _diffs_result(eng, ch, df)
        return res[:4] + (int(tot.value),) + res[4:]
    rc = eng.lib.dgr_sync_from(dst.ptr, dst_version, src.ptr, src_version, ms, C.byref(ch), C.byref(tot))
    if rc:
        return _err(rc)
    return _changed_result(eng, ch) + (int(tot.value),)


def sync_from_diffs(dst: State, dst_version: int, src: State, src_version: int, max_sync_size="infinite"):
    """sync_from that also returns on_diffs' list: {:ok, version', new_dots, changed, n_total, diffs}."""
    return sync_from(dst, dst_version, src, src_version, max_sync_size, _diffs=True)


def join_deltas(state: State, version: int, deltas, _diffs: bool = False):
    """deltas = [(dots, value, keys), ...]: the pending {:diff, delta, keys} messages of a
    replica's mailbox joined in ONE call (dgr_join_deltas: one packed message, one fold, the
    diff of the state before and after).  Same return shape as join_delta; `changed` is the
    batch's net change."""
    eng = state.engine
    hs = []
    for dots, value, _keys in deltas:  # pass 1: every value of the batch (a relabel re-spaces ids)
        for entries in value.values():
            for (v, _ts) in entries:
                eng.universe.value(eng.unwrap(v))
    for dots, value, keys in deltas:
        h = _Rows()
        _marshal_dots(eng, dots, h)
        _marshal_value(eng, value, h)
        hs.append((h, _marshal_keys(eng, keys)))
    if eng.lib.dgr_state_has_tree(state.ptr):
        rc = eng.refresh_terms()
        if rc:
            return _err(rc)
    k = len(hs)
    st = (dg_store * max(k, 1))(*[h.store() for h, _ in hs])
    cx = (dg_context * max(k, 1))(*[h.context() for h, _ in hs])
    kp = (C.c_void_p * max(k, 1))(*[kid.ctypes.data if len(kid) else None for _, kid in hs])
    kn = (C.c_uint64 * max(k, 1))(*[len(kid) for _, kid in hs])
    ch = dgr_changed()
    if _diffs:
        df = dgr_diffs()
        rc = eng.lib.dgr_join_deltas_diffs(state.ptr, version, k, st, cx, kp, kn, C.byref(ch), C.byref(df))
        return _err(rc) if rc else _diffs_result(eng, ch, df)
    rc = eng.lib.dgr_join_deltas(state.ptr, version, k, st, cx, kp, kn, C.byref(ch))
    if rc:
        return _err(rc)
    return _changed_result(eng, ch)


def join_deltas_diffs(state: State, version: int, deltas):
    """join_deltas that also returns on_diffs' list, NET over the batch (a key is reported
    once, with its read before the first and after the last delta; the callbacks the
    reference would have made per delta are not reproduced)."""
    return join_deltas(state, version, deltas, _diffs=True)


def mutate_batch(state: State, version: int, node, ops, _diffs: bool = False):
    """ops = [("add", key, value, ts) | ("remove", key)] in the order they were made"""
    eng = state.engine
    U, un = eng.universe, eng.unwrap
    nid = U.node(un(node))
    m = len(ops)
    kind = np.zeros(max(m, 1), np.uint8)
    key = np.zeros(max(m, 1), np.uint64)
    val = np.zeros(max(m, 1), np.uint64)
    ts = np.zeros(max(m, 1), np.int64)
    for op in ops:  # pass 1: values (a relabel re-spaces ids already handed out)
        if op[0] == "add":
            U.value(un(op[2]))
        elif op[0] != "remove":
            return ("error", (_abi.DG_E_INVAL, f"unknown op {op[0]!r}"))
    for i, op in enumerate(ops):
        key[i] = U.key(un(op[1]))
        if op[0] == "add":
            kind[i] = 1
            val[i] = U.value(un(op[2]))
            ts[i] = op[3]
    if eng.lib.dgr_state_has_tree(state.ptr):
        rc = eng.refresh_terms()
        if rc:
            return _err(rc)
    ch = dgr_changed()
    if _diffs:
        df = dgr_diffs()
        rc = eng.lib.dgr_mutate_batch_diffs(state.ptr, version, nid, m, kind.ctypes.data, key.ctypes.data,
                                            val.ctypes.data, ts.ctypes.data, C.byref(ch), C.byref(df))
        return _err(rc) if rc else _diffs_result(eng, ch, df)
    rc = eng.lib.dgr_mutate_batch(state.ptr, version, nid, m, kind.ctypes.data, key.ctypes.data,
                                  val.ctypes.data, ts.ctypes.data, C.byref(ch))
    if rc:
        return _err(rc)
    return _changed_result(eng, ch)


def mutate_batch_diffs(state: State, version: int, node, ops):
    """mutate_batch that also returns on_diffs' list for the batch's net changes
    (dgr_mutate_batch_diffs)."""
    return mutate_batch(state, version, node, ops, _diffs=True)


def read(state: State, version: int, keys):
    eng = state.engine
    all_ = isinstance(keys, str) and keys == "all"
    kid = np.zeros(1, np.uint64) if all_ else _marshal_keys(eng, keys)
    pk, pv, n = VP(), VP(), C.c_uint64()
    rc = eng.lib.dgr_read(state.ptr, version, 1 if all_ else 0, kid.ctypes.data,
                          0 if all_ else len(kid), C.byref(pk), C.byref(pv), C.byref(n))
    if rc:
        return _err(rc)
    k, v = _arr(pk, n.value, np.uint64), _arr(pv, n.value, np.uint64)
    U, w = eng.universe, eng.wrap
    return ("ok", {w(U.key_term(int(a))): _value_term(eng, b) for a, b in zip(k, v)})


def take(state: State, version: int, keys):
    eng = state.engine
    kid = _marshal_keys(eng, keys)
    out = dg_store()
    rc = eng.lib.dgr_take(state.ptr, version, kid.ctypes.data, len(kid), C.byref(out))
    if rc:
        return _err(rc)
    return ("ok", _unmarshal_rows(eng, out))


TAKE_BATCH_MAX = 64  # keysets per dgr_take_batch call (its masks are u64)


def _take_batch_raw(state: State, version: int, kids):
    """dgr_take_batch over marshalled keysets (at most TAKE_BATCH_MAX uint64 arrays): the
    return code and the raw dgr_taken (host views, valid until the engine's next call)."""
    eng = state.engine
    k = len(kids)
    kp = (VP * max(k, 1))(*[a.ctypes.data for a in kids])
    kn = (C.c_uint64 * max(k, 1))(*[len(a) for a in kids])
    tk = dgr_taken()
    rc = eng.lib.dgr_take_batch(state.ptr, version, k, kp, kn, C.byref(tk))
    return rc, tk


def take_batch(state: State, version: int, keysets):
    """take for k pending get_diff / send_diff messages as one call per 64 keysets
    (dgr_take_batch): ("ok", [value_map_0, ...]), element j what take(state, version,
    keysets[j])[1] is.  Every row of the union comes home and is unmarshalled ONCE; the
    messages that hold a key share its value map."""
    eng = state.engine
    keysets = list(keysets)
    out = []
    for c0 in range(0, len(keysets), TAKE_BATCH_MAX):
        kids = [_marshal_keys(eng, ks) for ks in keysets[c0:c0 + TAKE_BATCH_MAX]]
        rc, tk = _take_batch_raw(state, version, kids)
        if rc:
            return _err(rc)
        nu = int(tk.n_keys)
        masks, offs = _arr(tk.masks, nu, np.uint64), _arr(tk.offs, nu + 1, np.uint64)
        values = _unmarshal_rows(eng, tk.rows)  # {key term: entries}, every union row once
        ukeys = _arr(tk.keys, nu, np.uint64)
        held = [None] * nu  # per union key: (key term, its entries), None when the state lacks it
        for i in range(nu):
            if offs[i + 1] > offs[i]:
                kt = eng.wrap(eng.universe.key_term(int(ukeys[i])))
                held[i] = (kt, values[kt])
        for j in range(len(kids)):
            bit = 1 << j
            out.append({h[0]: h[1] for i, h in enumerate(held) if h is not None and int(masks[i]) & bit})
    return ("ok", out)


def merkle_build(state: State, version: int, depth: int):
    eng = state.engine
    rc = eng.refresh_terms() or eng.lib.dgr_merkle_build(state.ptr, version, depth)
    return "ok" if rc == 0 else _err(rc)


def merkle_prepare(state: State, version: int, levels: int):
    eng = state.engine
    p, n = VP(), C.c_uint64()
    rc = eng.lib.dgr_merkle_prepare(state.ptr, version, levels, C.byref(p), C.byref(n))
    if rc:
        return _err(rc)
    return ("continue", C.string_at(p, n.value))


def merkle_continue(state: State, version: int, cont: bytes, levels: int, max_sync):
    eng = state.engine
    rc = eng.refresh_terms()
    if rc:
        return _err(rc)
    mx = U64_MAX if max_sync == "infinite" else int(max_sync)
    status, p, n, pk, nk = C.c_int(), VP(), C.c_uint64(), VP(), C.c_uint64()
    rc = eng.lib.dgr_merkle_continue(state.ptr, version, cont, len(cont), levels, mx,
                                     C.byref(status), C.byref(p), C.byref(n), C.byref(pk),
                                     C.byref(nk))
    if rc:
        return _err(rc)
    if status.value == 1:
        return ("continue", C.string_at(p, n.value))
    return ("ok", [_key_term(eng, kid) for kid in _arr(pk, nk.value, np.uint64)])


CONT_BATCH_MAX = _abi.DG_CONT_BATCH_MAX  # messages per dgr_merkle_continue_batch call


def merkle_continue_batch(state: State, version: int, conts, levels: int, max_sync):
    """merkle_continue for k pending {:diff, %Diff{continuation: ...}} messages as one call per
    64 (dgr_merkle_continue_batch: one launch and one wait for the messages within the
    one-workgroup limits): ("ok", [r_0, ...]), r_j what merkle_continue(state, version,
    conts[j], levels, max_sync) is.  All answers are computed against the state as it is
    now.  A stale version fails the whole call."""
    eng = state.engine
    rc = eng.refresh_terms()
    if rc:
        return _err(rc)
    mx = U64_MAX if max_sync == "infinite" else int(max_sync)
    conts = list(conts)
    out = []
    for c0 in range(0, len(conts), CONT_BATCH_MAX):
        chunk = conts[c0:c0 + CONT_BATCH_MAX]
        k = len(chunk)
        bins = (C.c_char_p * k)(*chunk)
        lens = (C.c_uint64 * k)(*[len(c) for c in chunk])
        res = (dgr_cont_result * k)()
        rc = eng.lib.dgr_merkle_continue_batch(state.ptr, version, k, bins, lens, levels, mx, res)
        if rc:
            return _err(rc)
        for r in res:
            if r.rc:
                out.append(_err(r.rc))
            elif r.status == 1:
                out.append(("continue", C.string_at(r.bin, r.len)))
            else:
                out.append(("ok", [_key_term(eng, kid) for kid in _arr(r.keys, r.n_keys, np.uint64)]))
    return ("ok", out)


def merkle_continue_take_batch(state: State, version: int, conts, want, levels: int, max_sync):
    """merkle_continue_batch that also answers send_diff for the messages whose want[j] is set
    (the originator of a sync: diff.originator != diff.to): element j is ("ok", keys, value_map)
    where merkle_continue gives ("ok", keys) with keys, value_map what take(state, version, keys)[1]
    is; every other element is merkle_continue_batch's.  One call per 64 messages
    (dgr_merkle_continue_take_batch: the rows come out of the hops' own launch)."""
    eng = state.engine
    rc = eng.refresh_terms()
    if rc:
        return _err(rc)
    mx = U64_MAX if max_sync == "infinite" else int(max_sync)
    conts, want = list(conts), [1 if w else 0 for w in want]
    if len(want) != len(conts):
        return _err(_abi.DG_E_INVAL)
    out = []
    for c0 in range(0, len(conts), CONT_BATCH_MAX):
        chunk = conts[c0:c0 + CONT_BATCH_MAX]
        k = len(chunk)
        bins = (C.c_char_p * k)(*chunk)
        lens = (C.c_uint64 * k)(*[len(c) for c in chunk])
        res = (dgr_cont_result * k)()
        taken = (dgr_hop_rows * k)()
        rc = eng.lib.dgr_merkle_continue_take_batch(state.ptr, version, k, bins, lens, bytes(want[c0:c0 + k]),
                                                    levels, mx, res, taken)
        if rc:
            return _err(rc)
        for r, t, w in zip(res, taken, want[c0:c0 + k]):
            if r.rc:
                out.append(_err(r.rc))
            elif r.status == 1:
                out.append(("continue", C.string_at(r.bin, r.len)))
            else:
                keys = [_key_term(eng, kid) for kid in _arr(r.keys, r.n_keys, np.uint64)]
                out.append(("ok", keys, _unmarshal_rows(eng, t.rows)) if w and r.n_keys else ("ok", keys))
    return ("ok", out)


def sweep(engine: Engine, keys: bool = True):
    return engine.sweep(keys=keys)


def _key_term(eng: Engine, kid):
    """the key's term, or its placeholder when this node never interned it"""
    try:
        return eng.wrap(eng.universe.key_term(int(kid)))
    except KeyError:
        return eng.wrap(key_placeholder(kid))


def resolve_keys(engine: Engine, keys):
    """Placeholders of keys this node knows -> their terms (others stay placeholders):
    the originator's get_diff (causal_crdt.ex:112-123) takes its values of the keys a
    peer's continue_partial_diff named by id."""
    out = []
    for k in keys:
        t = engine.unwrap(k)
        if isinstance(t, tuple) and len(t) == 2 and isinstance(t[0], Atom) and t[0] == KEY_TAG:
            out.append(_key_term(engine, t[1]))
        else:
            out.append(k)
    return out


__all__ = ["engine_open", "state_load", "join_delta", "mutate_batch", "join_delta_diffs",
           "mutate_batch_diffs", "join_deltas", "join_deltas_diffs", "classify_diffs", "read", "take",
           "take_batch",
           "merkle_build", "merkle_prepare", "merkle_continue", "merkle_continue_batch", "merkle_continue_take_batch", "sweep", "resolve_keys", "key_placeholder",
           "Engine", "State", "DGR_E_STALE"]
