"""dg_join_delta's write on keys of several rows when NO key of the call changes its row
count (tests/inplace_cases.py; tests/test_inplace_cases.py proves on the oracle that writing
such a call in place in tuple order reads back rows it has just written, for 47 of its keys
in all three count tiles).  Every path that can serve the call -- the per-key join
(kdelta.hip + dg_kdw.h) through dg_join_delta_rows and dg_join_delta_diffs, the one-launch
small path (small.hip), the splice (DG_KD=0) -- against the C oracle's keyed join, bit for
bit: the state, the context, the changed keys, their rows, the diffs, and the tree against a
fresh build (apply() of test_gpu_join_delta.py, run() of test_gpu_lww_diffs.py).  Whether such
a call is written in place or through the spare store is the library's choice; that a call
whose changes are all one-row keys stays in place, and stays all or nothing, is not."""
import numpy as np
import pytest

import inplace_cases as IC
from delta_crdt_ex_amd.store import Engine, Store, u64
from test_gpu_join_delta import _assert_unchanged, _snapshot, apply, kdev, state_of, up
from test_gpu_lww_diffs import run
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu

KINDS = [IC.VV, IC.DOTS]
BASES = [IC.KVT - 4, IC.KVT]  # node ids in the count kernel's LDS tables, and past them


@pytest.mark.parametrize("with_tree", [False, True])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("kind", KINDS)
def test_count_preserving_multirow_keys(engine, kind, base, with_tree):
    """The 600-key call through join_delta(rows=...) and through join_delta_diffs."""
    c = IC.case(kind, base)
    apply(engine, c["state"], c["delta"], c["keys"], depth=10, with_tree=with_tree)
    _, cls = run(engine, c["state"], c["delta"], c["keys"], depth=10, with_tree=with_tree)
    # (every changed key has rows before and after; most of them read another value)
    assert cls["unchanged"] + cls["updated"] == len(c["random"]) + len(c["named"]) and cls["updated"] >= 50


@pytest.mark.parametrize("home", [False, True])
@pytest.mark.parametrize("name", list(IC.NAMED))
@pytest.mark.parametrize("kind,base", [(IC.VV, IC.KVT), (IC.DOTS, IC.KVT - 4)])
def test_named_key_alone(engine, kind, base, name, home):
    """One key, its delta rows, a context over its dots: the per-key join (any keyset with a VV
    state context takes it) and the small path, which merges from staged rows."""
    c = IC.case(kind, base)
    d, keys = IC.alone(c, name)
    st, _, _, wr = apply(engine, c["state"], d, keys, depth=10, home=home)
    x = c["named"][name]
    assert IC.key_rows(st.to_numpy(), x) == IC.key_rows(IC.joined(c)[0], x) == IC.key_rows(wr, x)


@pytest.mark.parametrize("kind", KINDS)
def test_splice_path(monkeypatch, kind):
    """DG_KD=0: the splice copies the keyset's rows from its edit store."""
    monkeypatch.setenv("DG_KD", "0")
    eng = Engine(0)
    try:
        c = IC.case(kind, IC.KVT - 4)
        apply(eng, c["state"], c["delta"], c["keys"], depth=10)
        run(eng, c["state"], c["delta"], c["keys"], depth=10)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_quiet_call_stays_in_place(engine, kind):
    """Only a one-row key changes, beside 400 unchanged keys of several rows: written in
    place (no swap), every other row bit for bit what it was."""
    c = IC.case(kind, IC.KVT - 4, "quiet")
    st, _, swapped, _ = apply(engine, c["state"], c["delta"], c["keys"], depth=10)
    assert not swapped
    before, after = c["state"]["rows"], st.to_numpy()
    rest = before[0] != np.uint64(c["named"]["one"])
    assert len(after[0]) == len(before[0]) and rest.sum() == len(before[0]) - 1
    for x, y in zip(after, before):
        assert np.array_equal(x[rest], y[rest])
    swapped, _ = run(engine, c["state"], c["delta"], c["keys"], depth=10)
    assert not swapped


@pytest.mark.parametrize("kind", KINDS)
def test_one_added_key_moves_the_rows(engine, kind):
    """The same multi-row keys with one key the state lacks: through the spare store."""
    c = IC.case(kind, IC.KVT - 4, "one_moves")
    _, _, swapped, _ = apply(engine, c["state"], c["delta"], c["keys"], depth=10)
    assert swapped
    swapped, _ = run(engine, c["state"], c["delta"], c["keys"], depth=10)
    assert swapped


@pytest.mark.parametrize("kind", KINDS)
def test_applied_twice_changes_nothing(engine, kind):
    c = IC.case(kind, IC.KVT)
    a, d, keys = c["state"], c["delta"], c["keys"]
    st, sc = state_of(a, extra_ctx=len(d["ctx"][1]))
    sd, cd = up(d)
    tree = engine.merkle_build(st, 10)
    c1, _ = engine.join_delta(st, sc, sd, cd, kdev(keys), Store.empty(st.n + sd.n, DEV), tree)
    root = tree.root()
    c2, sw2 = engine.join_delta(st, sc, sd, cd, kdev(keys), Store.empty(st.n + sd.n, DEV), tree)
    assert c1.numel() == len(c["random"]) + len(c["named"]) and c2.numel() == 0 and not sw2
    assert tree.root() == root
    wr, wc = IC.joined(c)
    rows_eq(st, wr)
    ctx_eq(sc, wc)
    fresh = engine.merkle_build(st, 10)
    assert np.array_equal(tree.nodes.cpu().numpy(), fresh.nodes.cpu().numpy())


@pytest.mark.parametrize("diffs", [False, True])
def test_failed_tree_update_with_multirow_keys(engine, diffs):
    """All or nothing: the call plus a one-row key outside the tree's key-hash shard that
    keeps its row count but changes (the tree was built over the shard's rows only) -- the
    shard error, and the state, its context and the tree are exactly what they were."""
    from delta_crdt_ex_amd._abi import DeltaGpuError
    c = IC.case(IC.VV, IC.KVT - 4, "outside")
    a, d, keys = c["state"], c["delta"], c["keys"]
    assert a["rows"][0][-1] == np.uint64(c["extra"])
    st, sc = state_of(a, extra_ctx=len(d["ctx"][1]))
    sd, cd = up(d)
    spare = Store.empty(st.n + sd.n, DEV)
    si, _ = up({"rows": tuple(col[:-1] for col in a["rows"]), "ctx": a["ctx"]})
    tree = engine.merkle_build(si, 8, shard_bits=1, shard=0)
    snap = _snapshot(st, sc, tree)
    join = engine.join_delta_diffs if diffs else engine.join_delta
    with pytest.raises(DeltaGpuError, match="shard"):
        join(st, sc, sd, cd, kdev(keys), spare, tree, rows=Store.empty(st.n + sd.n, DEV))
    _assert_unchanged(st, sc, tree, snap)
    # and the engine goes on: the same call without the tree
    apply(engine, a, d, keys, with_tree=False)
    assert u64(kdev(keys))[-1] == np.uint64(c["extra"])
