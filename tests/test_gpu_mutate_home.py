"""dg_mutate_home[_diffs] on cuda:0: a batch of one node's ops applied to the resident state in
one launch (csrc/small.hip, small_delta_kernel<.., true>).  Every case of mutate_home_cases.py
(checked with the oracle alone by test_mutate_home_cases.py) on twin states: one goes through
Engine.mutate_home_diffs, the other through Engine.mutate_batch + join_delta_home_diffs (or
join_delta_diffs where the home join's own limits decline the delta).  The twins' rows,
context, tree, `swapped`, changed keys, their rows and diffs are equal, the whole result block
is bit for bit the home join's where it served, both equal the oracle, and the tree equals a
fresh merkle_build of the new state.  Without a tree, with one, and on a shard tree.

A case meant to be served asserts that the call did serve it (a declined call would test the
old path); a case meant to be declined asserts DG_HOME_FALLBACK with the state, its context
and the tree byte for byte what they were, and that the two-step route then gives the
oracle's result."""
import numpy as np
import pytest
import torch

import mutate_home_cases as H
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd._abi import DeltaGpuError
from delta_crdt_ex_amd.store import Store, u64
from oracle import ref as R
from test_gpu_join_delta import _assert_unchanged, _snapshot, state_of
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu

DEPTH = 12
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
TREES = ("no_tree", "tree", "shard")
_ORACLE = {}


def _case(name, tree_mode="tree"):
    """the case and the oracle's answer, computed once and shared (read only)"""
    bits = 62 if tree_mode == "shard" else 63
    if (name, bits) not in _ORACLE:
        c = H.case(name, bits)
        _ORACLE[name, bits] = (c, H.oracle(c))
    return _ORACLE[name, bits]


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def ops_dev(ops):
    kind, key, val, ts, rank, n_adds = H.marshal(ops)
    kt = torch.from_numpy(kind).to(DEV) if len(ops) else torch.zeros(1, dtype=torch.uint8, device=DEV)
    return (kt, dev(key, np.int64), dev(val, np.int64), dev(ts, np.int64), dev(rank, np.int64), n_adds)


def _setup(eng, c, tree_mode, spare_extra=None, extra_ctx=1100):
    """(extra_ctx: room for the dot list the general join's check adds to the context's size)"""
    st, sc = state_of(c["a"], extra_ctx=extra_ctx)
    tree = None
    if tree_mode == "tree":
        tree = eng.merkle_build(st, DEPTH)
    elif tree_mode == "shard":
        tree = eng.merkle_build(st, DEPTH, shard_bits=2, shard=0)
    extra = len(c["ops"]) if spare_extra is None else spare_extra
    return st, sc, Store.empty(st.n + extra, DEV), tree


def _two_step(eng, c, st, sc, spare, tree):
    """mutate_batch + the home join, or the general join where the home join declines:
    (served by the home join, changed keys, (old, new, flags), swapped)"""
    d, dc, keys = eng.mutate_batch(st, sc, c["node"], *ops_dev(c["ops"]))
    got = eng.join_delta_home_diffs(st, sc, d, dc, keys, spare, tree)
    if got is not None:
        return True, got[0], got[4], got[3]
    changed, ov, nv, fl, sw = eng.join_delta_diffs(st, sc, d, dc, keys, spare, tree)
    return False, u64(changed), (u64(ov), u64(nv), fl.cpu().numpy()), sw


def _same(p, q):
    assert p.n == q.n
    for x, y in zip(p.to_numpy(), q.to_numpy()):
        assert np.array_equal(x, y)


def _same_tree(eng, tree, twin, st, tree_mode):
    assert torch.equal(tree.nodes, twin.nodes) and torch.equal(tree.counts, twin.counts)
    assert torch.equal(tree.starts, twin.starts) and tree.n_keys == twin.n_keys
    fresh = eng.merkle_build(st, DEPTH, shard_bits=2 if tree_mode == "shard" else 0, shard=0)
    assert torch.equal(tree.nodes, fresh.nodes) and torch.equal(tree.counts, fresh.counts)
    assert tree.n_keys == fresh.n_keys


SERVED = [n for n in H.CASES if H.CASES[n][4]]
SHARD = ("every", "one_update1", "one_absent_add", "in_place_one_moves", "large_state", "ops512")
# every served case without a tree and with one; the cases above on a shard tree too
TWINS = [(n, t) for n in SERVED for t in TREES if t != "shard" or n in SHARD]


@pytest.mark.parametrize("name,tree_mode", TWINS, ids=[f"{n}-{t}" for n, t in TWINS])
def test_mutate_home_twins(engine, name, tree_mode):
    c, o = _case(name, tree_mode)
    wr, wc, wch, want = o["rows"], o["ctx"], o["changed"], o["diffs"]
    block = engine.home_block()
    W = _abi.DG_HOME_WORDS
    # the twin: the two calls the new one replaces
    st2, sc2, spare2, tree2 = _setup(engine, c, tree_mode)
    block[:] = SENTINEL
    home2, changed2, diffs2, swapped2 = _two_step(engine, c, st2, sc2, spare2, tree2)
    words2 = block.copy()
    # the call
    st, sc, spare, tree = _setup(engine, c, tree_mode)
    block[:] = SENTINEL
    got = engine.mutate_home_diffs(st, sc, c["node"], *ops_dev(c["ops"]), spare, tree)
    assert got is not None and int(block[0]) == 0, "dg_mutate_home_diffs declined"
    changed, hrows, hctx, swapped, (ov, nv, fl) = got
    # ... against the twin
    assert swapped == swapped2 == c["moves"]
    assert np.array_equal(changed, changed2)
    for x, y in zip((ov, nv, fl), diffs2):
        assert np.array_equal(x, y)
    if home2:  # the home join served the delta: the whole block, header and diff ranges included
        assert np.array_equal(block, words2)
    else:
        assert "dots_over_1024" in c["must"]
    _same(st, st2)
    _same(sc, sc2)
    assert sc.kind == sc2.kind
    if tree is not None:
        _same_tree(engine, tree, tree2, st, tree_mode)
    # ... against the oracle
    rows_eq(st, wr)
    ctx_eq(sc, wc)
    assert np.array_equal(changed, wch)
    for what, x, y in zip(("old_val", "new_val", "flags"), (ov, nv, fl), want):
        assert np.array_equal(x, y), (what, x[:8], y[:8])
    sel = np.isin(wr[0], wch)
    for x, y in zip(hrows, wr):
        assert np.array_equal(x, y[sel])
    assert np.array_equal(hctx[0], wc[1]) and np.array_equal(hctx[1], wc[2])
    assert int(block[1]) == len(wch) and int(block[2]) == int(sel.sum()) and int(block[3]) == len(wc[1])
    n = len(wch)  # nothing past the changed keys' entries
    assert (block[_abi.DG_HOME_DIFF_OLD + n:_abi.DG_HOME_DIFF_NEW] == SENTINEL).all()
    assert (block[_abi.DG_HOME_DIFF_NEW + n:_abi.DG_HOME_DIFF_FLAGS] == SENTINEL).all()
    assert (block[_abi.DG_HOME_DIFF_FLAGS:].view(np.uint8)[n:] == 0xA5).all()
    if tree_mode != "tree":
        return
    # the plain call on a third copy: the same block without the diff ranges, the same state
    words = block.copy()
    st3, sc3, spare3, tree3 = _setup(engine, c, tree_mode)
    block[:] = SENTINEL
    plain = engine.mutate_home(st3, sc3, c["node"], *ops_dev(c["ops"]), spare3, tree3)
    assert plain is not None and int(block[0]) == 0, "dg_mutate_home declined"
    assert np.array_equal(block[:W], words[:W]) and (block[W:] == SENTINEL).all()
    assert plain[3] == swapped
    _same(st, st3)
    _same(sc, sc3)
    assert torch.equal(tree.nodes, tree3.nodes) and torch.equal(tree.counts, tree3.counts)


def _declined(engine, c, tree_mode, ops=None, spare_extra=None, dots_ctx=False, extra_ctx=1100):
    """The call declines and touches nothing."""
    a = c["a"]
    if dots_ctx:
        a = {"rows": a["rows"], "ctx": (R.DOTS,) + tuple(a["ctx"][1:])}
    st, sc, spare, tree = _setup(engine, dict(c, a=a), tree_mode, spare_extra, extra_ctx)
    snap = _snapshot(st, sc, tree) if tree is not None else None
    rows0, ctx0 = [x.copy() for x in st.to_numpy()], [x.copy() for x in sc.to_numpy()]
    block = engine.home_block()
    for f in (engine.mutate_home_diffs, engine.mutate_home):
        block[:] = SENTINEL
        assert f(st, sc, c["node"], *ops_dev(c["ops"] if ops is None else ops), spare, tree) is None
        assert int(block[0]) == _abi.DG_HOME_FALLBACK
        assert (block[_abi.DG_HOME_DIFF_OLD:] == SENTINEL).all()
        for x, y in zip(st.to_numpy() + sc.to_numpy(), rows0 + ctx0):
            assert np.array_equal(x, y)
        if tree is not None:
            _assert_unchanged(st, sc, tree, snap)
    return st, sc, spare, tree


@pytest.mark.parametrize("tree_mode", TREES[:2])
@pytest.mark.parametrize("name", [n for n in H.CASES if not H.CASES[n][4]])
def test_over_a_limit_is_declined_and_touches_nothing(engine, name, tree_mode):
    """513 ops, 1,025 state rows under the touched keys, node id 2048: DG_HOME_FALLBACK, nothing
    touched; mutate_batch and the general join then give the oracle's result on the same state."""
    c, o = _case(name)
    st, sc, spare, tree = _declined(engine, c, tree_mode)
    home, changed, diffs, _ = _two_step(engine, c, st, sc, spare, tree)
    rows_eq(st, o["rows"])
    ctx_eq(sc, o["ctx"])
    assert np.array_equal(changed, o["changed"])
    for x, y in zip(diffs, o["diffs"]):
        assert np.array_equal(x, y)


def _then_two_step(engine, c, o, st, sc, spare, tree):
    """... and the two calls then give the oracle's result on the state the decline left."""
    _, changed, diffs, _ = _two_step(engine, c, st, sc, spare, tree)
    rows_eq(st, o["rows"])
    ctx_eq(sc, o["ctx"])
    assert np.array_equal(changed, o["changed"])
    for x, y in zip(diffs, o["diffs"]):
        assert np.array_equal(x, y)


def test_other_declines_touch_nothing(engine):
    """A dot-set state context (dg_mutate_batch refuses it too: nothing to route to); a spare
    store one row short of state rows + touched keys; a context with no room for one more
    entry.  The last two then go through the two calls with the room those need."""
    c, o = _case("every")
    _declined(engine, c, "tree", dots_ctx=True)
    st, sc, spare, tree = _declined(engine, c, "tree", spare_extra=len(o["touched"]) - 1)
    _then_two_step(engine, c, o, st, sc, Store.empty(st.n + len(c["ops"]), DEV), tree)
    st, sc, spare, tree = _declined(engine, c, "tree", extra_ctx=0)
    room, _ = state_of(c["a"], extra_ctx=1100)[1], None
    room.node[: sc.n].copy_(sc.node[: sc.n])
    room.cnt[: sc.n].copy_(sc.cnt[: sc.n])
    _then_two_step(engine, c, o, st, room, spare, tree)
    # a spare of exactly state rows + touched keys and a context with room for one entry serve
    st, sc, spare, tree = _setup(engine, c, "tree", spare_extra=len(o["touched"]), extra_ctx=1)
    assert engine.mutate_home_diffs(st, sc, c["node"], *ops_dev(c["ops"]), spare, tree) is not None
    rows_eq(st, o["rows"])


@pytest.mark.parametrize("tree_mode", TREES[:2])
def test_unsorted_ops_are_refused_with_nothing_changed(engine, tree_mode):
    c, o = _case("every")
    st, sc, spare, tree = _setup(engine, c, tree_mode)
    snap = _snapshot(st, sc, tree) if tree is not None else None
    kind, key, val, ts, rank, n_adds = ops_dev(c["ops"])
    key = key.clone()
    key[[3, 9]] = key[[9, 3]]
    for f in (engine.mutate_home, engine.mutate_home_diffs):
        with pytest.raises(DeltaGpuError, match="sorted") as ei:
            f(st, sc, c["node"], kind, key, val, ts, rank, n_adds, spare, tree)
        assert ei.value.code == _abi.DG_E_ORDER
        rows_eq(st, c["a"]["rows"])
        ctx_eq(sc, c["a"]["ctx"])
        if tree is not None:
            _assert_unchanged(st, sc, tree, snap)
    # ... and the engine serves the sorted batch afterwards
    assert engine.mutate_home_diffs(st, sc, c["node"], *ops_dev(c["ops"]), spare, tree) is not None
    rows_eq(st, o["rows"])


def test_ops_in_page_locked_host_memory(engine):
    """The ops read in place from dg_host_alloc memory, as the replica layer passes them."""
    import ctypes as C
    c, o = _case("every")
    kind, key, val, ts, rank, n_adds = H.marshal(c["ops"])
    m = len(kind)
    p = C.c_void_p()
    assert engine.lib.dg_host_alloc(engine.h, 4 * 8 * m + m, C.byref(p)) == 0
    words = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(4 * m,))
    words[:m], words[m:2 * m], words[2 * m:3 * m], words[3 * m:] = key, val, ts.view(np.uint64), rank
    kb = np.ctypeslib.as_array(C.cast(p.value + 32 * m, C.POINTER(C.c_uint8)), shape=(m,))
    kb[:] = kind
    st, sc, spare, tree = _setup(engine, c, "tree")
    ss, xc, sp, t = st.abi(), sc.abi(), spare.abi(), tree.abi()
    sw = C.c_int(0)
    block = engine.home_block()
    engine._order()
    rc = engine.lib.dg_mutate_home(engine.h, C.byref(ss), C.byref(xc), c["node"], m, p.value + 32 * m,
                                   C.cast(p.value, _abi.P64), C.cast(p.value + 8 * m, _abi.P64),
                                   C.cast(p.value + 16 * m, _abi.PI64), C.cast(p.value + 24 * m, _abi.P64), n_adds,
                                   C.byref(sp), C.byref(t), engine._home, C.byref(sw))
    assert rc == 0 and int(block[0]) == 0
    engine._commit_join(st, sc, spare, tree, ss, xc, t, sw.value)
    rows_eq(st, o["rows"])
    ctx_eq(sc, o["ctx"])
    assert np.array_equal(block[_abi.DG_HOME_KEYS:_abi.DG_HOME_KEYS + int(block[1])], o["changed"])
    engine.lib.dg_host_free(engine.h, p)


def _patched(name, rows=None, ctx=None):
    """A copy of case `name` with a column entry of its first one-row touched key's state row,
    or a context counter, replaced (the row keeps its place: its key has one row)."""
    c = dict(_case(name)[0])
    r = [x.copy() for x in c["a"]["rows"]]
    x = (c["a"]["ctx"][0], c["a"]["ctx"][1].copy(), c["a"]["ctx"][2].copy())
    if rows is not None:
        col, value = rows
        key = c["keys"][c["recipes"].index("update1")]
        i = np.flatnonzero(r[0] == key)
        assert len(i) == 1
        r[col][i[0]] = value
    if ctx is not None:
        node, value = ctx
        i = np.flatnonzero(x[1] == node)
        assert len(i) == 1
        x[2][i[0]] = value
    c["a"] = {"rows": tuple(r), "ctx": x}
    return c


U64_MAX = (1 << 64) - 1


@pytest.mark.parametrize("tree_mode", TREES[:2])
def test_declines_made_in_the_kernel(engine, tree_mode):
    """What only the kernel can see: a taken row by node 2048 (2047 is served), a taken row
    whose counter is 2^64 - 1, the VV's counter of `node` at 2^64 - 1, and C[node] + n_adds
    reaching 2^64 - 1 (one less is served).  Declined: nothing touched."""
    # (node2047's recipes: absent_add, update1 -- two adds by node 2047 / 5)
    c = _patched("node2047", rows=(3, 2048))
    st, sc, spare, tree = _declined(engine, c, tree_mode)
    _then_two_step(engine, c, H.oracle(c), st, sc, spare, tree)  # (the general join has no such limit)
    _declined(engine, _patched("node2047", rows=(4, U64_MAX)), tree_mode)
    _declined(engine, _patched("node2047", ctx=(2047, U64_MAX)), tree_mode)
    _declined(engine, _patched("node2047", ctx=(2047, U64_MAX - 2)), tree_mode)  # + 2 adds
    for c in (_patched("node2047", rows=(3, 2047)), _patched("node2047", ctx=(2047, U64_MAX - 3))):
        o = H.oracle(c)
        st, sc, spare, tree = _setup(engine, c, tree_mode)
        got = engine.mutate_home_diffs(st, sc, c["node"], *ops_dev(c["ops"]), spare, tree)
        assert got is not None, "declined inside its limits"
        rows_eq(st, o["rows"])
        ctx_eq(sc, o["ctx"])
        assert np.array_equal(got[0], o["changed"])
        if tree is not None:
            fresh = engine.merkle_build(st, DEPTH)
            assert torch.equal(tree.nodes, fresh.nodes) and tree.n_keys == fresh.n_keys


@pytest.mark.parametrize("tree_mode", TREES[:2])
def test_an_empty_batch_is_served_and_changes_nothing(engine, tree_mode):
    c, _ = _case("every")
    st, sc, spare, tree = _setup(engine, c, tree_mode)
    snap = _snapshot(st, sc, tree) if tree is not None else None
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    block = engine.home_block()
    for f in (engine.mutate_home, engine.mutate_home_diffs):
        block[:] = SENTINEL
        got = f(st, sc, c["node"], torch.zeros(0, dtype=torch.uint8, device=DEV), e, e, e, e, 0, spare, tree)
        assert got is not None and int(block[0]) == 0
        assert len(got[0]) == 0 and not got[3] and [int(x) for x in block[1:3]] == [0, 0]
        rows_eq(st, c["a"]["rows"])
        ctx_eq(sc, c["a"]["ctx"])
        if tree is not None:
            _assert_unchanged(st, sc, tree, snap)
