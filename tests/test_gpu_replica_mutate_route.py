"""dgr_mutate_batch's two routes (c_src/replica_join.c): DGR_MUTATE_ROUTE=home tries
dg_mutate_home on the packed message first and falls through to the copy, dg_mutate_batch and
the join when it declines; =batch is that sequence alone.  A history of one-key ops, a 300-op
batch and a 600-op batch (over the home call's 512: not tried) run through nif.py under each
route on an engine of its own, on a state with a tree: both routes return the same changed
keys, diffs, context and version steps and leave the same rows, reads and tree, and the
engine's counters (dgr_mutate_route_stats) say which route ran.  Removes of keys with more
rows than the first dot capacity allows take the copy route's second attempt and give what
one-op calls give.  And
causal_crdt.update_resident_state_with_ops against apply_ops on a non-resident twin."""
import os

import numpy as np
import pytest

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle.erlterm import tg
from test_gpu_replica_deltas import _twin
from test_gpu_replica_diffs import _peer

pytestmark = pytest.mark.gpu

ROUTES = ("home", "batch")


class route:
    """One "BEAM node" whose engine was opened with DGR_MUTATE_ROUTE=name."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("gpu tests need an MI355X: torch.cuda.is_available() is False")
        self.saved = (B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS, os.environ.get("DGR_MUTATE_ROUTE"))
        B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = 0, 0
        os.environ["DGR_MUTATE_ROUTE"] = self.name
        try:
            B.GPU.load_nif(0)
        finally:
            if self.saved[2] is None:
                del os.environ["DGR_MUTATE_ROUTE"]
            else:
                os.environ["DGR_MUTATE_ROUTE"] = self.saved[2]
        assert B.GPU.engine() is not None
        return self

    def stats(self):
        return B.GPU.engine().mutate_route_stats()

    def __exit__(self, *exc):
        B.GPU.close()
        B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = self.saved[:2]


def _history():
    """[(diffs?, ops)]: one-key adds, updates and removes (present and absent keys), then a
    300-op batch with repeated keys, two empty batches, then 600 ops."""
    one = [[("add", tg(1000), tg("new"), 5)], [("add", tg(7), tg("upd"), 6)], [("remove", tg(8))],
           [("remove", tg(5000))], [("add", tg(7), tg("upd"), 7)], [("add", tg(1000), tg("again"), -4)]]
    big = []
    for i in range(300):
        k = tg((i * 7) % 450)
        big.append(("add", k, tg(("v", i)), 100 + i) if i % 4 else ("remove", k))
    over = [("add", tg(2000 + i % 500), tg(("w", i)), 900 + i) for i in range(600)]
    return [(i % 2 == 0, ops) for i, ops in enumerate(one)] + [(True, big), (False, big[:40]), (True, []), (False, []), (True, over)]


def _run(name):
    base = _peer([1], list(range(400)), lambda j, i: ("base", i), 100)
    out = []
    with route(name) as node:
        res, ver = _twin(base)
        for diffs, ops in _history():
            f = nif.mutate_batch_diffs if diffs else nif.mutate_batch
            r = f(res, ver, tg("n2"), ops)
            assert r[0] == "ok" and r[1] == ver + 1, r
            ver = r[1]
            out.append((r[2:], node.stats()))
        keys = [tg(i) for i in range(450)] + [tg(1000), tg(5000)] + [tg(2000 + i) for i in range(500)]
        final = (nif.read(res, ver, "all"), nif.take(res, ver, keys), nif.merkle_prepare(res, ver, B.LEVELS))
    return out, final


def test_both_routes_give_the_same():
    got = {name: _run(name) for name in ROUTES}
    (oh, fh), (ob, fb) = got["home"], got["batch"]
    assert [x[0] for x in oh] == [x[0] for x in ob]
    assert fh == fb
    # every batch of at most 512 ops was tried and served; the 600-op batch was not tried
    n = len(oh)
    assert [x[1] for x in oh] == [(i + 1, i + 1, 0) for i in range(n - 1)] + [(n - 1, n - 1, 0)]
    assert all(x[1] == (0, 0, 0) for x in ob)
    assert oh[-2][1][1] > 0


def _removes(name, base, keys, slice_len, diffs):
    """`keys` of `base` removed under route `name`, slice_len ops to a call: (changed keys and
    diffs of all calls, the final reads, rows and tree, the route's counters)"""
    ops = [("remove", tg(k)) for k in keys]
    changed, dd = [], []
    with route(name) as node:
        res, ver = _twin(base)
        f = nif.mutate_batch_diffs if diffs else nif.mutate_batch
        for i in range(0, len(ops), slice_len):
            r = f(res, ver, tg("n2"), ops[i:i + slice_len])
            assert r[0] == "ok" and r[1] == ver + 1, r
            ver = r[1]
            changed += r[3]
            dd += r[4] if diffs else []
        stats = node.stats()
        final = (nif.read(res, ver, "all"), nif.take(res, ver, [tg(k) for k in keys]),
                 nif.merkle_prepare(res, ver, B.LEVELS))
    return sorted(changed, key=repr), sorted(dd, key=repr), final, stats


def test_more_state_dots_than_the_first_dot_capacity():
    """dgr_mutate_batch asks dg_mutate_batch_async for 8m + n_adds + 1 context dots and, on
    DG_E_CAPACITY, once more for state rows + n_adds + 1.  Removes of keys with more than 8 rows
    each need the second: one 12-row key (12 > 9; and one 26-row key, past the 16 entries of
    slack the buffer's first allocation adds) under `batch`, and 600 keys of 9 rows (5,400 >
    4,801; over the home call's 512 ops, so not tried) under both routes.  The same changed
    keys, diffs, reads, rows and tree as a twin that takes the ops one to a call (9 <= 8 + 1:
    no retry), and the counters say which route ran."""
    for n_nodes in (12, 26):
        base = _peer(list(range(1, n_nodes + 1)), list(range(8)), lambda j, i: ("v", j, i), 100)
        assert all(len(v) == n_nodes for v in base.value.values()) and n_nodes > 8 * 1 + 0 + 1
        one = _removes("batch", base, [3], 1, True)
        twin = _removes("home", base, [3], 1, True)  # (dg_mutate_home: no dot list to size)
        assert one[:3] == twin[:3] and len(one[0]) == 1 and one[1] == [("remove", tg(3))]
        assert one[3] == (0, 0, 0) and twin[3] == (1, 1, 0)
    base = _peer(list(range(1, 10)), list(range(600)), lambda j, i: ("v", j, i), 100)
    assert all(len(v) == 9 for v in base.value.values()) and 600 * 9 > 8 * 600 + 0 + 1 + 16
    keys = [(i * 7) % 600 for i in range(600)]  # (batch order is not key order)
    for name in ROUTES:
        one = _removes(name, base, keys, 600, True)
        twin = _removes(name, base, keys, 1, True)
        assert one[:3] == twin[:3]
        assert len(one[0]) == 600 and all(v is None for _, v in one[0]) and len(one[1]) == 600
        assert one[2][0] == ("ok", {})
        assert one[3] == (0, 0, 0)
        assert twin[3] == ((600, 600, 0) if name == "home" else (0, 0, 0))
    plain = _removes("batch", base, keys, 600, False)
    assert plain[0] == one[0] and plain[2] == one[2]


def test_update_resident_state_with_ops_equals_apply_ops():
    """The resident counterpart of apply_ops: the same diffs, the same journal record as the
    delta route writes, the same rows and context as the non-resident twin."""
    from delta_crdt_ex_amd import aw_lww_map as M
    from delta_crdt_ex_amd import causal_crdt as CC
    from delta_crdt_ex_amd.store import Store

    class Recorder:
        """storage.Journal's append side: what would be written"""
        sequence_number = 41

        def __init__(self):
            self.records = []

        def append(self, seq, changed, rows, ctx, root=None):
            self.records.append((seq, np.asarray(changed).tolist(), [np.asarray(c).tolist() for c in rows],
                                 (ctx[0], np.asarray(ctx[1]).tolist(), np.asarray(ctx[2]).tolist()), root))

    def fresh():
        st = M.compress_dots(M.new())
        for i in range(40):
            st = M.join(st, M.add(i, i * 10, "n1", st, ts=i), [i])
        return st

    ops = [("add", 3, 33, 100), ("remove", 4), ("add", 4, 44, 101), ("add", 3, 333, 102), ("remove", 5),
           ("add", 99, 9, 103), ("remove", 99), ("add", 7, 70, 104), ("add", 8, 80, 8), ("remove", 777)]
    twin, want = CC.apply_ops(fresh(), ops, "n2")
    got, recs = {}, {}
    for how in ("ops", "delta"):
        st = fresh()
        spare = Store.empty(st.rows.n + 64, st.rows.device)
        tree = M.engine().merkle_build(st.rows, 8)
        j = Recorder()
        if how == "ops":
            got[how] = CC.update_resident_state_with_ops(st, ops, "n2", spare, tree, j)
        else:
            delta, keys = M.mutate_batch(ops, "n2", st)
            got[how] = CC.update_resident_state_with_delta(st, delta, keys, spare, tree, j)
        for x, y in zip(st.rows.to_numpy() + st.ctx.to_numpy(), twin.rows.to_numpy() + twin.ctx.to_numpy()):
            assert np.array_equal(x, y)
        recs[how] = (tree.root(), tree.n_keys, j.records)
    assert got["ops"] == got["delta"] == want and want
    assert recs["ops"] == recs["delta"] and len(recs["ops"][2]) == 1 and recs["ops"][2][0][0] == 42
