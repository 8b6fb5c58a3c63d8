"""on_diffs served by the device-resident replica, through the NIF's mirror
(delta_crdt_ex_amd/nif.py -> c_src/replica_join.c dgr_join_delta_diffs / dgr_mutate_batch_diffs ->
dg_join_delta_home_diffs or dg_join_delta_diffs): the diffs list every call returns equals
diffs_to_callback/3's rule (causal_crdt.ex:361-381) applied to the term oracle's reads
before and after -- and a replica that uses ONLY those lists, reading no old struct,
delivers the `received` streams of CPU-only replicas."""
import pytest
from hypothesis import HealthCheck, given, settings

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle import awlww_term as T
from oracle.erlterm import tg
from hypothesis import strategies as st
from test_gpu_binding import STEP, Clock

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_node():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need an MI355X: torch.cuda.is_available() is False")
    saved = (B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS)
    B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = 0, 0
    B.GPU.load_nif(0)
    assert B.GPU.engine() is not None
    yield
    B.GPU.close()
    B.GPU_MIN_DOTS, B.GPU_MIN_READ_KEYS = saved


def reference_diffs(before, after, keys):
    """diffs_to_callback/3 over the term oracle's reads (each key once)."""
    keys = list(dict.fromkeys(keys))
    old, new = B.read_cpu(before, keys), B.read_cpu(after, keys)
    nil, out = tg(None), []
    for key in keys:
        o, n = old.get(key, nil), new.get(key, nil)  # Map.get: absent -> nil
        if o == n:
            continue  # {old, old}
        out.append(("remove", key) if n == nil else ("add", key, n))
    return out


def _norm(diffs):
    return sorted(map(repr, diffs))


class Resident:
    """One device state with a tree, and the term oracle's state beside it."""

    def __init__(self):
        self.terms = B.compress_dots(B.new())
        st = B.attach_gpu(self.terms, 0)
        assert st.gpu is not None
        self.res, self.ver, _ = st.gpu
        self.calls = 0

    def _check(self, r, after, keys):
        assert r[0] == "ok", r
        _, self.ver, dots, changed, diffs = r
        want_changed = B.diff(self.terms, after, list(dict.fromkeys(keys)))
        assert {k for k, _ in changed} == {d[1] for d in want_changed}
        for k, v in changed:
            assert v == after.value.get(k)
        assert _norm(diffs) == _norm(reference_diffs(self.terms, after, keys)), (self.calls, diffs[:4])
        # ascending key-id order: the order of `changed`
        order = [k for k, _ in changed]
        assert [d[1] for d in diffs] == [k for k in order if k in {d[1] for d in diffs}]
        assert dots == after.dots
        self.terms = after
        self.calls += 1
        return diffs

    def mutate(self, node, ops):
        """ops = [("add", key, value, ts) | ("remove", key)] (plain terms) as ONE batch"""
        node = tg(node)
        ops = [(op[0], tg(op[1])) + ((tg(op[2]), op[3]) if op[0] == "add" else ()) for op in ops]
        after = self.terms
        for op in ops:
            d = B.add(op[1], op[2], node, after, op[3]) if op[0] == "add" else B.remove(op[1], node, after)
            after = B.join_cpu(after, d, [op[1]])
        r = nif.mutate_batch_diffs(self.res, self.ver, node, ops)
        return self._check(r, after, [op[1] for op in ops])

    def join(self, delta, keys):
        after = B.join_cpu(self.terms, delta, keys)
        r = nif.join_delta_diffs(self.res, self.ver, delta.dots, delta.value, list(keys))
        return self._check(r, after, keys)


def _peer(nodes, keys, value_of, ts0):
    """a CPU replica's state after each of `nodes` added every key (concurrently: one entry
    per node and key survives the join)"""
    out = B.compress_dots(B.new())
    for j, node in enumerate(nodes):
        one = B.compress_dots(B.new())
        for i, k in enumerate(keys):
            d = B.add(tg(k), tg(value_of(j, i)), tg(node), one, ts0 + i)
            one = B.join_cpu(one, d, [tg(k)])
        out = B.join_cpu(out, one, list(one.value))
    return out


def test_history_of_diffs_calls():
    """One-key ops, a 600-key batch, 600 overwrites that add no key (the large path in place)
    and a 2,000-key sync delta of three entries per key (the large path with moves; its changed
    rows overflow the return block: grow and re-take), then small calls again on the same
    engine; values include nil, 1 and 1.0, tuples."""
    r = Resident()
    ts = iter(range(1000, 10 ** 9))
    vals = [None, 1, 1.0, (1, 2), "x", b"y", True]
    # one-key ops: adds, the same value again, nil, 1 -> 1.0, removes, a remove of nothing
    seen = []
    for i in range(40):
        seen.append(r.mutate(1, [("add", i % 8, vals[i % len(vals)], next(ts))]))
    seen.append(r.mutate(1, [("add", 3, 1, next(ts))]))
    seen.append(r.mutate(1, [("add", 3, 1.0, next(ts))]))           # 1 =/= 1.0: an add
    assert seen[-1] == [("add", tg(3), tg(1.0))] and tg(1.0) != tg(1)
    seen.append(r.mutate(1, [("add", 3, 1.0, next(ts))]))           # the same value: changed, no diff
    assert seen[-1] == []
    seen.append(r.mutate(1, [("add", 3, None, next(ts))]))          # nil: a remove
    assert seen[-1] == [("remove", tg(3))]
    seen.append(r.mutate(1, [("remove", 3)]))                        # {nil, nil}
    assert seen[-1] == []
    seen.append(r.mutate(1, [("remove", 3)]))                        # nothing changed at all
    assert seen[-1] == []
    seen.append(r.mutate(1, [("add", 5, (1, 2), next(ts)), ("remove", 5), ("add", 5, (2, 1), next(ts))]))
    assert seen[-1] == [("add", tg(5), tg((2, 1)))]
    assert any(d and d[0][0] == "remove" for d in seen) and any(d and d[0][0] == "add" for d in seen)
    # a 600-key batch: 560 new keys, overwrites and removes of old ones (the large path, rows move)
    ops = [("add", 100 + i, vals[i % len(vals)], next(ts)) for i in range(560)]
    ops += [("add", i, i, next(ts)) for i in range(0, 8, 2)] + [("remove", i) for i in range(1, 8, 2)]
    ops += [("add", 1000 + i, None, next(ts)) for i in range(36)]
    assert len({op[1] for op in ops}) == 604
    d = r.mutate(1, ops)
    assert len(d) > 400
    # 600 overwrites of keys that are all there, one entry each: no key is added and no row
    # count changes, so the large path writes in place; every key reads another value
    ops = [("add", 100 + i, vals[(i + 1) % len(vals)], next(ts)) for i in range(560)]
    ops += [("add", i, "z", next(ts)) for i in range(0, 8, 2)] + [("add", 1000 + i, i, next(ts)) for i in range(36)]
    assert len({op[1] for op in ops}) == 600 and all(len(r.terms.value[tg(op[1])]) == 1 for op in ops)
    d = r.mutate(1, ops)
    assert len(d) == 600
    # a sync delta of 2,000 keys, three concurrent entries per key, 560 of them known here
    keys = list(range(100, 2100))
    peer = _peer([2, 3, 4], keys, lambda j, i: (j, i) if i % 3 else float(i), 500)
    d = r.join(B.detach(peer), [tg(k) for k in keys])
    assert len(d) > 1400
    # small calls after the block grew: a three-entry key collapses to one, goes, comes back
    assert r.mutate(1, [("add", 150, "mine", next(ts))]) == [("add", tg(150), tg("mine"))]
    assert r.mutate(1, [("remove", 150)]) == [("remove", tg(150))]
    assert r.mutate(1, [("add", 150, "mine", next(ts))]) == [("add", tg(150), tg("mine"))]
    # a small sync delta (a VV context): the one-launch path
    small = _peer([7], [150, 151, 9000], lambda j, i: -i, 10 ** 9)
    d = r.join(B.detach(small), [tg(150), tg(151), tg(9000)])
    assert len(d) == 3
    ok, got = nif.read(r.res, r.ver, "all")
    assert ok == "ok" and got == B.read_cpu(r.terms)


class DiffsReplica(B.Replica):
    """INTEGRATION.md §3.3's patch: update_state_with_delta sends every delta to the device
    (a local mutation as mutate_batch_diffs, a sync delta as join_delta_diffs) and hands
    on_diffs the returned list.  No old struct is kept or read for the callback."""

    def update_state_with_delta(self, delta, keys):
        st = self.crdt_state
        assert st.gpu is not None and not st.gpu[2]
        res, ver, _ = st.gpu
        if B.is_mapset(delta.dots):
            r = nif.mutate_batch_diffs(res, ver, B.op_node(delta) or self.node_id, B.delta_ops(delta, keys))
        else:
            r = nif.join_delta_diffs(res, ver, delta.dots, delta.value, list(keys))
        assert r[0] == "ok", r
        _, ver2, dots, changed, diffs = r
        self.crdt_state = B.apply_changed(st, (res, ver2, ()), dots, changed)
        self.diffs_to_callback(changed, diffs)
        self.write_to_storage()

    def diffs_to_callback(self, changed, diffs):  # :359-381, the case already decided
        if not changed:
            return None
        self.received.append(diffs)
        if self.on_diffs:
            self.on_diffs(diffs)
        return diffs


def test_subscriber_receives_diffs():  # delta_subscriber_test.exs:11-28
    r = DiffsReplica(1, Clock())
    r.mutate("add", "Derek", "Kraan")
    assert r.received[-1] == [("add", tg("Derek"), tg("Kraan"))]
    r.mutate("add", "Derek", "Kraan")  # refute_received: same value, new dot
    assert r.received[-1] == []
    r.mutate("add", "Derek", None)  # add k nil -> {:remove, k} (:26-27)
    assert r.received[-1] == [("remove", tg("Derek"))]
    assert len(r.received) == 3 and r.crdt_state.gpu[2] == ()
    assert r.read() == B.read_cpu(r.crdt_state) == {tg("Derek"): tg(None)}


def test_updates_are_bundled():  # delta_subscriber_test.exs:49-77
    c = Clock()
    c1, c2 = DiffsReplica(1, c), DiffsReplica(2, c)
    for k in ("Derek", "Andrew", "Nathan"):
        c1.mutate("add", k, "Kraan")
    c2.received.clear()
    c1.sync_to(c2)
    assert len(c2.received) == 1, c2.received
    assert {k: v for _, k, v in c2.received[0]} == {tg("Derek"): tg("Kraan"), tg("Andrew"): tg("Kraan"),
                                                    tg("Nathan"): tg("Kraan")}
    assert c2.read() == c1.read()


def _run(cls, steps, **kw):
    c = Clock()
    rs = (cls(1, c, **kw), cls(2, c, **kw))
    for op, who, k, v in steps:
        if op == "sync":
            rs[who].sync_to(rs[1 - who])
        else:
            rs[who].mutate(op, k, *(() if op == "remove" else (v,)))
    return rs


@settings(max_examples=10, deadline=None, suppress_health_check=list(HealthCheck))
@given(st.lists(STEP, min_size=1, max_size=18))
def test_histories_deliver_the_reference_streams(steps):
    """INTEGRATION.md §3.4's property: mutations interleaved with sync rounds on two replicas
    that take on_diffs from the device equal the same history on two CPU-only replicas --
    `received` callback for callback (each list compared sorted: the reference leaves the
    order inside one list open), reads and raw states."""
    g = _run(DiffsReplica, steps)
    p = _run(B.Replica, steps, gpu=False)
    for a, b in zip(g, p):
        assert [_norm(x) for x in a.received] == [_norm(x) for x in b.received]
        assert B.read(a.crdt_state) == B.read_cpu(b.crdt_state)
        assert T.canon(T.AW(a.crdt_state.dots, a.crdt_state.value)) == \
            T.canon(T.AW(b.crdt_state.dots, b.crdt_state.value))
        assert a.crdt_state.gpu is not None
