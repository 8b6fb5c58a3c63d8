"""dgr_join_deltas' two routes (c_src/replica_join.c): DGR_DELTAS_ROUTE=keyed tries
dg_join_deltas_keyed first and falls through to dg_join_deltas when it declines, =stream is
the streaming call alone.  test_gpu_replica_deltas' batches and its draining replica run
through nif.py under each route on an engine of its own (the route is read at engine open):
both routes return the same changed keys, diffs, context and version steps, leave the same
rows and tree, and converge with the CPU-only replicas -- also over a run of batches on one
state whose middle batch the keyed call declines (a delta row outside its keyset).  Which
route ran is read from the engine's counters (dgr_deltas_route_stats): under =keyed every batch
is tried and served or declined as the case expects, under =stream none is tried."""
import os

import pytest

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle import awlww_term as T
from oracle.erlterm import tg
from test_gpu_replica_deltas import SHAPES, DrainingReplica, _batch, _history, _twin
from test_gpu_replica_diffs import _norm, _peer, reference_diffs

pytestmark = pytest.mark.gpu

ROUTES = ("keyed", "stream")


class route:
    """One "BEAM node" whose engine was opened with DGR_DELTAS_ROUTE=name."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        import torch
        if not torch.cuda.is_available():
            pytest.fail("gpu tests need an MI355X: torch.cuda.is_available() is False")
        self.saved = (B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS, os.environ.get("DGR_DELTAS_ROUTE"))
        B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = 0, 0
        os.environ["DGR_DELTAS_ROUTE"] = self.name
        try:
            B.GPU.load_nif(0)
        finally:
            if self.saved[2] is None:
                del os.environ["DGR_DELTAS_ROUTE"]
            else:
                os.environ["DGR_DELTAS_ROUTE"] = self.saved[2]
        assert B.GPU.engine() is not None
        return self

    def stats(self):
        """(tried, served, declined) of this node's engine"""
        return B.GPU.engine().deltas_route_stats()

    def __exit__(self, *exc):
        B.GPU.close()
        B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = self.saved[:2]


def _one_batch(base, batch):
    """The batch into a fresh twin of `base`: everything the call returns and leaves."""
    res, ver = _twin(base)
    r = nif.join_deltas_diffs(res, ver, [(d.dots, d.value, keys) for d, keys in batch])
    assert r[0] == "ok", r
    _, ver2, dots, changed, diffs = r
    allkeys = list(dict.fromkeys(list(base.value) + [k for _, keys in batch for k in keys]))
    return {"step": ver2 - ver, "dots": dots, "changed": changed, "diffs": diffs,
            "rows": nif.take(res, ver2, allkeys), "read": nif.read(res, ver2, "all"),
            "tree": nif.merkle_prepare(res, ver2, B.LEVELS)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_both_routes_give_the_same(shape):
    base = _peer([1], list(range(400)), lambda j, i: ("base", i), 100)
    batch = _batch(SHAPES[shape])
    got, stats = {}, {}
    for name in ROUTES:
        with route(name) as node:
            got[name] = _one_batch(base, batch)
            stats[name] = node.stats()
    assert stats == {"keyed": (1, 1, 0), "stream": (0, 0, 0)}  # sync deltas: VV contexts, rows in their keysets
    assert got["keyed"] == got["stream"]
    terms = base
    for delta, keys in batch:
        terms = B.join_cpu(terms, delta, keys)
    g = got["keyed"]
    assert g["step"] == 1 and g["dots"] == terms.dots and g["read"] == ("ok", B.read_cpu(terms))
    assert g["rows"] == ("ok", terms.value)
    union = list(dict.fromkeys(k for _, keys in batch for k in keys))
    assert _norm(g["diffs"]) == _norm(reference_diffs(base, terms, union)) and len(g["diffs"]) > 0


def test_a_declined_batch_mid_stream():
    """Three batches on one state; the second has a delta whose keyset lacks one of its rows'
    keys (the right-biased carry: only the streaming call joins it), so the keyed route falls
    back for that batch alone."""
    base = _peer([1], list(range(300)), lambda j, i: ("base", i), 100)
    batches = [_batch([(0, 60), (40, 60)]), _batch([(100, 50), (120, 50)]), _batch([(200, 40), (250, 80)])]
    d, keys = batches[1][0]
    batches[1][0] = (d, keys[:-1])  # the last key's row stays in the delta
    assert tg(149) in d.value and tg(149) not in batches[1][0][1]
    got, stats = {}, {}
    for name in ROUTES:
        with route(name) as node:
            res, ver = _twin(base)
            out = []
            for batch in batches:
                r = nif.join_deltas_diffs(res, ver, [(x.dots, x.value, ks) for x, ks in batch])
                assert r[0] == "ok" and r[1] == ver + 1, r
                ver = r[1]
                out.append(r[2:])
                stats.setdefault(name, []).append(node.stats())
            got[name] = (out, nif.read(res, ver, "all"), nif.merkle_prepare(res, ver, B.LEVELS))
    assert stats == {"keyed": [(1, 1, 0), (2, 1, 1), (3, 2, 1)], "stream": [(0, 0, 0)] * 3}
    assert got["keyed"] == got["stream"]
    terms = base
    for batch in batches:
        for delta, ks in batch:
            terms = B.join_cpu(terms, delta, ks)
    assert got["keyed"][1] == ("ok", B.read_cpu(terms)) and got["keyed"][0][-1][0] == terms.dots


@pytest.mark.parametrize("name", ROUTES)
def test_a_draining_replica_converges_with_cpu_replicas(name):
    with route(name) as node:
        target, peers = _history(DrainingReplica)
        before = B.detach(target.crdt_state)
        for p in peers:
            p.sync_to(target)
        n, diffs = target.drain()
        assert n == 3 and node.stats() == ((1, 1, 0) if name == "keyed" else (0, 0, 0))
        cpu, cpu_peers = _history(B.Replica, gpu=False)
        for p in cpu_peers:
            p.sync_to(cpu)
        assert B.read(target.crdt_state) == B.read_cpu(cpu.crdt_state)
        assert T.canon(T.AW(target.crdt_state.dots, target.crdt_state.value)) == \
            T.canon(T.AW(cpu.crdt_state.dots, cpu.crdt_state.value))
        keys = list(dict.fromkeys(list(before.value) + list(cpu.crdt_state.value)))
        assert _norm(diffs) == _norm(reference_diffs(before, cpu.crdt_state, keys))
        res, ver, _ = target.crdt_state.gpu
        assert nif.read(res, ver, "all") == ("ok", B.read_cpu(target.crdt_state))
