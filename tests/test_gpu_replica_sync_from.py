"""One anti-entropy exchange between two replicas resident on ONE engine, device to device, through
the NIF's mirror (delta_crdt_ex_amd/nif.py sync_from[_diffs] -> c_src/replica_join.c dgr_sync_from
-> dg_merkle_diff_take, then the join of the rows where they stand).

The term oracle: keys = the keys whose raw value maps differ, by ascending key id, the first
max_sync of them; the result is join(dst, %{dots: src.dots, value: Map.take(src.value, keys)}, keys).
Compared: dst's full read and rows, the changed list, the new dots, the version step, and the tree
(merkle_prepare's bytes equal those of a replica freshly loaded from the expected terms)."""
import pytest

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle.erlterm import tg
from test_gpu_replica_diffs import _norm, _peer, gpu_node, reference_diffs  # noqa: F401 (gpu_node: the fixture)

pytestmark = pytest.mark.gpu

_pairs = {}


def pair(size):
    """(src, dst) term states of one history: a common base, then each side's own adds, overwrites
    (also with nil) and removes -- keys on one side only, keys on both with other entries, keys
    left alone.  `size`: how many keys the source touched."""
    if size not in _pairs:
        n_base = 300
        base = _peer([1], list(range(n_base)), lambda j, i: ("base", i), 100)
        ps = _peer([2], list(range(200, 200 + size)), lambda j, i: ("s", i) if i % 5 else None, 1000)
        src = B.join_cpu(base, ps, list(ps.value))
        for k in (3, 7, 205):
            src = B.join_cpu(src, B.remove(tg(k), tg(2), src), [tg(k)])
        pd = _peer([3], list(range(250, 340)), lambda j, i: ("d", i), 2000)
        dst = B.join_cpu(base, pd, list(pd.value))
        for k in (5, 7, 260):
            dst = B.join_cpu(dst, B.remove(tg(k), tg(3), dst), [tg(k)])
        _pairs[size] = (src, dst)
    return _pairs[size]


def attach(terms):
    st = B.attach_gpu(terms, 0)
    assert st.gpu is not None
    return st.gpu[0], st.gpu[1]


def differing(eng, a, b):
    """the keys whose raw value maps differ, ascending by key id"""
    keys = [k for k in dict.fromkeys(list(a.value) + list(b.value)) if a.value.get(k) != b.value.get(k)]
    ids = nif._marshal_keys(eng, keys)
    return [k for _, k in sorted(zip(ids.tolist(), keys), key=lambda p: p[0])]


def expected(eng, dst, src, max_sync):
    keys = differing(eng, dst, src)
    kept = keys if max_sync is None else keys[:max_sync]
    delta = B.AW(src.dots, {k: src.value[k] for k in kept if k in src.value})
    return B.join_cpu(dst, delta, kept), kept, len(keys)


def check_round(rd, vd, dst, rs, vs, src, max_sync, diffs=False):
    """one sync_from against the oracle; returns (version, the expected terms, n_total)"""
    eng = rd.engine
    exp, kept, total = expected(eng, dst, src, max_sync)
    f = nif.sync_from_diffs if diffs else nif.sync_from
    r = f(rd, vd, rs, vs, "infinite" if max_sync is None else max_sync)
    assert r[0] == "ok", r
    _, v2, dots, changed, n_total = r[:5]
    assert n_total == total
    assert v2 == (vd + 1 if kept else vd)
    assert dots == exp.dots
    want = [k for k in kept if dst.value.get(k) != exp.value.get(k)]
    assert [k for k, _ in changed] == want  # (ascending key id, as the kept keys are)
    for k, v in changed:
        assert v == exp.value.get(k)
    if diffs:
        assert _norm(r[5]) == _norm(reference_diffs(dst, exp, kept))
    allkeys = list(dict.fromkeys(list(dst.value) + list(src.value)))
    assert nif.read(rd, v2, "all") == ("ok", B.read_cpu(exp))
    assert nif.take(rd, v2, allkeys) == ("ok", exp.value)
    fresh, vf = attach(exp)
    assert nif.merkle_prepare(rd, v2, B.LEVELS) == nif.merkle_prepare(fresh, vf, B.LEVELS)
    # the source and its version are untouched
    assert nif.read(rs, vs, "all") == ("ok", B.read_cpu(src))
    return v2, exp, total


@pytest.mark.parametrize("size", [60, 700])  # a delta in the one-workgroup join's range, one over 512 keys
@pytest.mark.parametrize("max_sync", [1, None])
def test_one_exchange_against_the_term_oracle(size, max_sync):
    src, dst = pair(size)
    (rs, vs), (rd, vd) = attach(src), attach(dst)
    _, _, total = check_round(rd, vd, dst, rs, vs, src, max_sync)
    assert total > (512 if size == 700 else 1)


def test_rounds_of_200_in_both_directions_converge():
    src, dst = pair(700)
    (rs, vs), (rd, vd) = attach(src), attach(dst)
    for rounds in range(1, 12):
        vd, dst, t1 = check_round(rd, vd, dst, rs, vs, src, 200)
        vs, src, t2 = check_round(rs, vs, src, rd, vd, dst, 200)
        if t1 == 0 and t2 == 0:
            break
    assert t1 == 0 and t2 == 0 and rounds > 2
    assert nif.read(rd, vd, "all") == nif.read(rs, vs, "all")
    # equal replicas: no version step, nothing changed
    r = nif.sync_from(rd, vd, rs, vs, 200)
    assert r[0] == "ok" and r[1] == vd and r[3] == [] and r[4] == 0


def test_the_diffs_are_join_delta_diffs_on_a_twin():
    """sync_from_diffs' diffs equal join_delta_diffs' on a twin of dst given the same delta through
    the term path."""
    src, dst = pair(60)
    (rs, vs), (rd, vd), (rt, vt) = attach(src), attach(dst), attach(dst)
    exp, kept, total = expected(rd.engine, dst, src, None)
    r = nif.sync_from_diffs(rd, vd, rs, vs, "infinite")
    t = nif.join_delta_diffs(rt, vt, src.dots, {k: src.value[k] for k in kept if k in src.value}, kept)
    assert r[0] == "ok" and t[0] == "ok"
    assert r[1:4] == t[1:4] and r[4] == total and r[5] == t[4]
    assert len(r[5]) > 0
    check_round(*attach(dst), dst, rs, vs, src, None, diffs=True)


def test_stale_versions_and_a_state_without_a_tree():
    src, dst = pair(60)
    (rs, vs), (rd, vd) = attach(src), attach(dst)
    assert nif.sync_from(rd, vd + 1, rs, vs, "infinite") == ("error", "stale")
    assert nif.sync_from(rd, vd, rs, vs + 1, "infinite") == ("error", "stale")
    assert nif.sync_from_diffs(rd, vd - 1, rs, vs, 5) == ("error", "stale")
    r = nif.sync_from(rd, vd, rd, vd, "infinite")  # dst == src
    assert r[0] == "error" and r[1][0] == nif._abi.DG_E_INVAL
    ok, bare, vb = nif.state_load(rd.engine, src.dots, src.value)  # no merkle_build
    assert ok == "ok"
    for a, b in (((rd, vd), (bare, vb)), ((bare, vb), (rs, vs))):
        r = nif.sync_from(a[0], a[1], b[0], b[1], "infinite")
        assert r[0] == "error" and r[1][0] == nif._abi.DG_E_INVAL
    ok, flat, vf = nif.state_load(rd.engine, src.dots, src.value)  # a tree of another depth
    assert ok == "ok" and nif.merkle_build(flat, vf, B.MERKLE_DEPTH - 2) == "ok"
    r = nif.sync_from(rd, vd, flat, vf, "infinite")
    assert r[0] == "error" and r[1][0] == nif._abi.DG_E_INVAL
    for bad in (0, -3, "many"):
        assert nif.sync_from(rd, vd, rs, vs, bad)[0] == "error"
    # nothing was touched: the exchange still runs from the versions as they were
    check_round(rd, vd, dst, rs, vs, src, None)
