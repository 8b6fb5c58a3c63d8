"""A batch of sync deltas through the device-resident replica, through the NIF's mirror
(delta_crdt_ex_amd/nif.py join_deltas_diffs -> c_src/replica_join.c dgr_join_deltas_diffs ->
dg_join_deltas): twin states, one taking the batch in one call and one taking the same
deltas one by one, end in the same rows, context and tree; the batch's diffs are the NET
diffs (the term oracle's read before the first and after the last delta, classified as
diffs_to_callback/3 does); an older version is refused; and a replica that drains three
neighbours' deltas in one call ends where CPU-only replicas end.

As in test_gpu_replica_diffs.py, every one-by-one call that takes the large path (more than
512 keys) adds at least one key the state lacks (see that file's header)."""
import pytest

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle import awlww_term as T
from oracle.erlterm import tg
from test_gpu_binding import Clock
from test_gpu_replica_diffs import _norm, _peer, gpu_node, reference_diffs  # noqa: F401 (gpu_node: the fixture)

pytestmark = pytest.mark.gpu


def _twin(terms):
    st = B.attach_gpu(terms, 0)
    assert st.gpu is not None
    return st.gpu[0], st.gpu[1]


def _batch(shape):
    """[(delta, keys)]: sync deltas of CPU peers (VV contexts), overlapping key ranges."""
    out = []
    for j, (lo, n) in enumerate(shape):
        keys = list(range(lo, lo + n))
        peer = _peer([10 + j], keys, lambda _j, i, j=j: (j, i) if i % 4 else float(i), 500 + 10 * j)
        out.append((B.detach(peer), [tg(k) for k in keys]))
    return out


SHAPES = {
    # k = 3: 100 keys (the one-launch path one by one), then 700 and 600 (the large path)
    "k3": [(0, 100), (50, 700), (700, 600)],
    # k = 20: 30 keys each, 600 in all (each small, the batch over 512), overlapping by 10
    "k20": [(20 * i, 30) for i in range(20)],
    # k = 3 and fewer than 512 keys in all
    "k3 small": [(0, 40), (30, 40), (390, 40)],
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_twin_states(shape):
    base = _peer([1], list(range(400)), lambda j, i: ("base", i), 100)
    batch = _batch(SHAPES[shape])
    (ra, va), (rb, vb) = _twin(base), _twin(base)
    # one by one
    terms = base
    for delta, keys in batch:
        r = nif.join_delta_diffs(rb, vb, delta.dots, delta.value, keys)
        assert r[0] == "ok", r
        vb, dots_b = r[1], r[2]
        terms = B.join_cpu(terms, delta, keys)
    assert dots_b == terms.dots
    # the batch: ONE version step
    r = nif.join_deltas_diffs(ra, va, [(d.dots, d.value, keys) for d, keys in batch])
    assert r[0] == "ok", r
    _, va2, dots_a, changed, diffs = r
    assert va2 == va + 1 and vb == va + len(batch)
    assert dots_a == dots_b
    union = list(dict.fromkeys(k for _, keys in batch for k in keys))
    allkeys = list(dict.fromkeys(list(base.value) + union))
    ta, tb = nif.take(ra, va2, allkeys), nif.take(rb, vb, allkeys)
    assert ta[0] == "ok" and ta == tb and ta[1] == terms.value
    assert nif.read(ra, va2, "all") == nif.read(rb, vb, "all") == ("ok", B.read_cpu(terms))
    assert nif.merkle_prepare(ra, va2, B.LEVELS) == nif.merkle_prepare(rb, vb, B.LEVELS)
    # the net change and the net diffs: first old, last new
    want = {k for k in allkeys if base.value.get(k) != terms.value.get(k)}
    assert {k for k, _ in changed} == want and len(changed) == len(want)
    for k, v in changed:
        assert v == terms.value.get(k)
    assert _norm(diffs) == _norm(reference_diffs(base, terms, union))
    assert len(diffs) > 0
    # the plain call on a third twin gives the same state
    rc, vc = _twin(base)
    r3 = nif.join_deltas(rc, vc, [(d.dots, d.value, keys) for d, keys in batch])
    assert r3[0] == "ok" and r3[1:] == (vc + 1, dots_a, changed)


def test_stale_version_is_refused():
    base = _peer([1], list(range(50)), lambda j, i: i, 100)
    batch = [(d.dots, d.value, keys) for d, keys in _batch([(0, 10), (5, 10)])]
    res, ver = _twin(base)
    r = nif.join_deltas_diffs(res, ver, batch)
    assert r[0] == "ok" and r[1] == ver + 1
    assert nif.join_deltas_diffs(res, ver, batch) == ("error", "stale")
    assert nif.join_deltas(res, ver, batch) == ("error", "stale")
    assert nif.read(res, ver + 1, "all")[0] == "ok"  # the state is where the first call left it
    # an empty batch changes nothing and keeps the version
    r0 = nif.join_deltas_diffs(res, ver + 1, [])
    assert r0[0] == "ok" and r0[1] == ver + 1 and r0[3] == [] and r0[4] == []


class DrainingReplica(B.Replica):
    """INTEGRATION.md §3's handle_info patch: {:diff, delta, keys} messages are collected
    from the mailbox and joined in ONE join_deltas_diffs call; on_diffs gets the net list."""

    def __init__(self, *a, **kw):
        self.mailbox = []
        super().__init__(*a, **kw)

    def handle(self, msg):
        if msg[0] == "diff" and len(msg) == 3:
            self.mailbox.append((msg[1], list(msg[2])))
            return []
        return super().handle(msg)

    def drain(self):
        ok, st = B.flush(self.crdt_state)
        assert ok == "ok", st
        res, ver, _ = st.gpu
        r = nif.join_deltas_diffs(res, ver, [(d.dots, d.value, keys) for d, keys in self.mailbox])
        assert r[0] == "ok", r
        _, ver2, dots, changed, diffs = r
        n = len(self.mailbox)
        self.mailbox = []
        self.crdt_state = B.apply_changed(st, (res, ver2, ()), dots, changed)
        if changed:
            self.received.append(diffs)
        return n, diffs


def _history(cls_target, **kw):
    c = Clock()
    target = cls_target(1, c, **kw)
    peers = [B.Replica(n, c, **kw) for n in (2, 3, 4)]
    for i in range(30):
        target.mutate("add", i, ("t", i))
    for j, p in enumerate(peers):
        for i in range(10 * j, 10 * j + 25):  # overlapping keys, also with the target's
            p.mutate("add", i, (j, i) if i % 5 else None)
        p.mutate("remove", 10 * j + 3)
    return target, peers


def test_a_replica_drains_three_neighbours_deltas_in_one_call():
    target, peers = _history(DrainingReplica)
    before = B.detach(target.crdt_state)
    for p in peers:
        p.sync_to(target)
    assert len(target.mailbox) == 3
    n, diffs = target.drain()
    assert n == 3
    # the same history on CPU-only replicas, each delta applied as it arrives
    cpu, cpu_peers = _history(B.Replica, gpu=False)
    for p in cpu_peers:
        p.sync_to(cpu)
    assert B.read(target.crdt_state) == B.read_cpu(cpu.crdt_state)
    assert T.canon(T.AW(target.crdt_state.dots, target.crdt_state.value)) == \
        T.canon(T.AW(cpu.crdt_state.dots, cpu.crdt_state.value))
    keys = list(dict.fromkeys(list(before.value) + list(cpu.crdt_state.value)))
    assert _norm(diffs) == _norm(reference_diffs(before, cpu.crdt_state, keys))
    assert target.crdt_state.gpu is not None and target.crdt_state.gpu[2] == ()
    # the device agrees with the struct's terms
    res, ver, _ = target.crdt_state.gpu
    assert nif.read(res, ver, "all") == ("ok", B.read_cpu(target.crdt_state))
