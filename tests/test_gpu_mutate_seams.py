"""dg_mutate_batch on cuda:0 where random batches never get: the tile seams (a group's last op
in the next tile, a tile without a head), the last tile's offset scan past one round of 256
tiles, the generator's grid-stride loop, the dot list's no-sort paths, removes alone, the
node's counter found at every place of the VV, 64-bit counters and 32-bit node ids through
the two radix sorts, and the capacity refusal that the wrappers retry.  Every case of
mutate_batch_cases.py (checked with the oracle alone by test_mutate_batch_cases.py): the
delta's rows, its dot list in order and the touched keys equal ref.mutate_batch's, and the
join with the touched keys equals ref.join2's.  All values are integers, compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import mutate_batch_cases as M
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd._abi import DeltaGpuError
from delta_crdt_ex_amd.store import Context, Store, _ptr, u64
from oracle import ref as R
from test_gpu_mutate_home import dev, ops_dev
from test_gpu_parity import DEV, ctx_eq, rows_eq, up

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _case(name):
    """the case and the oracle's answer, computed once and shared (read only)"""
    if name not in _ORACLE:
        c = M.case(name)
        _ORACLE[name] = (c, M.oracle(c, join=name != "wide_dots"))
    return _ORACLE[name]


def _served(engine, name, ops=None):
    """Engine.mutate_batch gives the oracle's delta, dot list and touched keys"""
    c, o = _case(name)
    s, x = up(c["a"])
    d, dots, keys = engine.mutate_batch(s, x, c["node"], *(ops_dev(c["ops"]) if ops is None else ops))
    rows_eq(d, o["delta"])
    assert np.array_equal(u64(keys), o["touched"])
    if name != "own_dot":
        ctx_eq(dots, o["dots"])
    return s, x, d, dots, keys


@pytest.mark.parametrize("name", M.NAMES)
def test_case(engine, name):
    c, o = _case(name)
    s, x, d, dots, keys = _served(engine, name)
    if name == "own_dot":
        # a touched key's state row carries a dot the batch generates: the kernel lists it
        # twice (it sorts, it does not deduplicate), the oracle's set once
        assert dots.kind == R.DOTS
        node, cnt = dots.to_numpy()
        assert np.all((node[1:] > node[:-1]) | ((node[1:] == node[:-1]) & (cnt[1:] >= cnt[:-1])))
        assert sorted(set(zip(node.tolist(), cnt.tolist()))) == list(zip(o["dots"][1].tolist(), o["dots"][2].tolist()))
        assert dots.n == len(o["dots"][1]) + 3
    if name == "wide_dots":  # (its point is the sort; the join's node-id limits are another file's subject)
        return
    out, octx = engine.join2(s, x, d, dots, keys=keys)
    rows_eq(out, o["rows"])
    ctx_eq(octx, o["ctx"])


# ---------------------------------------------------------------- the raw call

PAD = 64


def _a5(t):
    t.view(torch.uint8).fill_(0xA5)
    return t


class _Raw:
    """dg_mutate_batch through the library, into output buffers PAD entries larger than the
    result and filled with 0xA5, with the capacities the caller states"""

    def __init__(self, engine, c, o):
        self.engine, self.c, self.o = engine, c, o
        self.s, self.x = up(c["a"])
        self.ops = ops_dev(c["ops"])
        self.m = len(c["ops"])
        self.n_keys, self.n_rows = len(o["touched"]), len(o["delta"][0])
        self.n_dots = int(np.isin(c["a"]["rows"][0], o["touched"]).sum()) + self.ops[5]

    def call(self, keys_cap, delta_cap, dots_cap, n_adds=None):
        e = self.engine
        self.out = Store.empty(self.n_keys + PAD, DEV)  # (delta rows <= touched keys)
        for col in (self.out.key, self.out.val, self.out.ts, self.out.node, self.out.cnt):
            _a5(col)
        self.dots = Context.empty(R.DOTS, self.n_dots + PAD, DEV)
        _a5(self.dots.node), _a5(self.dots.cnt)
        self.keys = _a5(torch.empty(self.n_keys + PAD, dtype=torch.int64, device=DEV))
        assert keys_cap <= self.keys.numel() and delta_cap <= self.out.cap and dots_cap <= self.dots.cap
        kind, key, val, ts, rank, adds = self.ops
        ss, xs, so, xd = self.s.abi(), self.x.abi(), self.out.abi(), self.dots.abi()
        so.cap, xd.cap = delta_cap, dots_cap
        nk = C.c_uint64(0xA5)
        e._order()
        rc = e.lib.dg_mutate_batch(e.h, C.byref(ss), C.byref(xs), self.c["node"], self.m, _ptr(kind, C.c_void_p),
                                   _ptr(key, _abi.P64), _ptr(val, _abi.P64), _ptr(ts, _abi.PI64), _ptr(rank, _abi.P64),
                                   adds if n_adds is None else n_adds, C.byref(so), C.byref(xd),
                                   _ptr(self.keys, _abi.P64), keys_cap, C.byref(nk))
        self.so, self.xd, self.nk = so, xd, nk.value
        return rc

    def untouched_from(self, n_keys, n_rows, n_dots):
        for t, n in [(self.keys, n_keys), (self.dots.node, n_dots), (self.dots.cnt, n_dots)] + \
                [(col, n_rows) for col in (self.out.key, self.out.val, self.out.ts, self.out.node, self.out.cnt)]:
            assert bool((t[n:].view(torch.uint8) == 0xA5).all())

    def refused(self, keys_cap, delta_cap, dots_cap):
        """DG_E_CAPACITY, a message that names the three sizes, no output written"""
        assert self.call(keys_cap, delta_cap, dots_cap) == _abi.DG_E_CAPACITY
        msg = (self.engine.lib.dg_last_error() or b"").decode()
        assert f"needs {self.n_keys} keys, {self.n_rows} delta rows, {self.n_dots} context dots" in msg, msg
        self.untouched_from(0, 0, 0)
        assert self.nk == 0xA5 and self.so.n == 0 and self.xd.n == 0

    def ok(self, keys_cap, delta_cap, dots_cap):
        """DG_OK, the oracle's result, nothing at or past n_keys, delta.n, dots.n written"""
        o = self.o
        assert self.call(keys_cap, delta_cap, dots_cap) == _abi.DG_OK
        assert (self.nk, self.so.n, self.xd.n) == (self.n_keys, self.n_rows, self.n_dots)
        assert self.xd.kind == R.DOTS
        self.out._set(self.so)
        self.dots._set(self.xd)
        rows_eq(self.out, o["delta"])
        ctx_eq(self.dots, o["dots"])
        assert np.array_equal(u64(self.keys[:self.nk]), o["touched"])
        self.untouched_from(self.n_keys, self.n_rows, self.n_dots)


def test_raw_call_writes_its_result_and_nothing_more(engine):
    c, o = _case("group600")
    r = _Raw(engine, c, o)
    assert r.n_dots == len(o["dots"][1]) and 0 < r.n_rows < r.n_keys
    r.ok(r.n_keys + PAD, r.n_rows + PAD, r.n_dots + PAD)


@pytest.mark.parametrize("which", ["keys_cap", "delta_cap", "dots_cap"])
def test_raw_call_capacities(engine, which):
    """One short of the touched keys, the delta rows, state dots + n_adds: refused with nothing
    written, and the engine then serves a plain call; exactly that many: served."""
    c, o = _case("group600")
    r = _Raw(engine, c, o)
    full = {"keys_cap": r.n_keys, "delta_cap": r.n_rows, "dots_cap": r.n_dots}
    assert all(v > 0 for v in full.values())
    r.refused(**dict(full, **{which: full[which] - 1}))
    _served(engine, "group600")
    r.ok(**full)
    _served(engine, "group600")
    if which == "delta_cap":  # ... and a delta store of one row per touched key
        r.ok(**dict(full, delta_cap=r.n_keys))


def test_capacity_retry_through_the_engine(engine):
    """many_rows_few_ops: 120 state dots under 3 removes.  The wrapper's first capacity, 8m +
    n_adds + 1 = 25, is refused (shown through the raw call); Engine.mutate_batch comes back
    with the oracle's result from its second; the engine serves the next case."""
    c, o = _case("many_rows_few_ops")
    r = _Raw(engine, c, o)
    first = 8 * r.m + r.ops[5] + 1
    assert first == 25 < r.n_dots == 120 <= r.s.n + r.ops[5] + 1
    r.refused(r.n_keys, max(r.n_rows, 1), first)
    s, x, d, dots, keys = _served(engine, "many_rows_few_ops")
    assert dots.n == 120
    out, octx = engine.join2(s, x, d, dots, keys=keys)
    rows_eq(out, o["rows"])
    ctx_eq(octx, o["ctx"])
    _served(engine, "m257")


# ---------------------------------------------------------------- errors

def _swapped(ops, i, j):
    """the marshalled ops with sorted positions i and j exchanged"""
    kind, key, val, ts, rank, n_adds = M.marshal(ops)
    for col in (kind, key, val, ts, rank):
        col[[i, j]] = col[[j, i]]
    assert key[i] > key[j]
    kt = torch.from_numpy(kind).to(DEV)
    return (kt, dev(key, np.int64), dev(val, np.int64), dev(ts, np.int64), dev(rank, np.int64), n_adds)


@pytest.mark.parametrize("name,i", [("m257", 255), ("tiles257", 65_535)])
def test_order_error_across_a_tile_seam(engine, name, i):
    """Positions 255 | 256 of m257 and the last two ops of tiles257 (the last is alone in tile
    256) exchanged: the descending pair lies in two tiles.  Refused; the sorted batch is served."""
    c, _ = _case(name)
    assert (i + 1) % M.TILE == 0 and i + 1 < len(c["ops"])
    s, x = up(c["a"])
    with pytest.raises(DeltaGpuError, match="sorted") as ei:
        engine.mutate_batch(s, x, c["node"], *_swapped(c["ops"], i, i + 1))
    assert ei.value.code == _abi.DG_E_ORDER
    _served(engine, name)


def test_argument_errors(engine):
    c, _ = _case("m257")
    s, x = up(c["a"])
    kind, key, val, ts, rank, n_adds = ops_dev(c["ops"])
    with pytest.raises(DeltaGpuError, match="n_adds > m") as ei:
        engine.mutate_batch(s, x, c["node"], kind, key, val, ts, rank, len(c["ops"]) + 1)
    assert ei.value.code == _abi.DG_E_INVAL
    _served(engine, "m257")
    x.kind = R.DOTS
    with pytest.raises(DeltaGpuError, match="version vector") as ei:
        engine.mutate_batch(s, x, c["node"], kind, key, val, ts, rank, n_adds)
    assert ei.value.code == _abi.DG_E_INVAL
    _served(engine, "m257")
