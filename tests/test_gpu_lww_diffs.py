"""dg_join_delta_diffs and dg_read_diff on cuda:0: on_diffs' LWW reads of the changed keys
before and after a resident join (diffs_to_callback/3, causal_crdt.ex:361-381), bit-equal
to the C oracle's read/2 of the oracle's rows before and after its keyed join, on every path
of dg_join_delta (the per-key join in place and with moves, the splice, the full join);
the join itself equal to what dg_join_delta_rows gives on a second copy."""
import ctypes as C

import numpy as np
import pytest
import torch

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.store import Engine, Store, u64
from lww_diffs_cases import NEW, OLD, classes, expected_diffs
from oracle import ref as R
from test_gpu_join_delta import _assert_unchanged, _runs_state, _snapshot, kdev, state_of, up
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu


def _setup(eng, a, d, depth, with_tree):
    st, sc = state_of(a, extra_ctx=len(d["ctx"][1]))
    sd, cd = up(d)
    tree = eng.merkle_build(st, depth) if with_tree else None
    return st, sc, sd, cd, Store.empty(st.n + sd.n, DEV), tree, Store.empty(st.n + sd.n, DEV)


def _np(t):
    return t.cpu().numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint64)


def run(eng, a, d, keys, depth=10, with_tree=True):
    """join_delta_diffs against the oracle (the join, the changed keys, their diffs) and
    against join_delta(rows=...) on a second copy (state, context, changed keys and rows,
    tree -- bit for bit).  Returns (swapped, the changed keys' classes)."""
    keys = np.unique(np.asarray(keys, np.uint64))
    st, sc, sd, cd, spare, tree, rows = _setup(eng, a, d, depth, with_tree)
    changed, ov, nv, fl, swapped = eng.join_delta_diffs(st, sc, sd, cd, kdev(keys), spare, tree, rows=rows)
    wr, wc = R.join2(a["rows"], a["ctx"], d["rows"], d["ctx"], keys=keys)
    wch = R.changed_keys(a["rows"], wr, keys)
    assert np.array_equal(u64(changed), wch)
    want = expected_diffs(a["rows"], wr, wch)
    got = (_np(ov), _np(nv), _np(fl))
    for name, x, y in zip(("old_val", "new_val", "flags"), got, want):
        assert np.array_equal(x, y), name
    rows_eq(st, wr)
    ctx_eq(sc, wc)
    st2, sc2, sd2, cd2, spare2, tree2, rows2 = _setup(eng, a, d, depth, with_tree)
    changed2, swapped2 = eng.join_delta(st2, sc2, sd2, cd2, kdev(keys), spare2, tree2, rows=rows2)
    assert swapped2 == swapped and torch.equal(changed, changed2)
    for p, q in ((st, st2), (sc, sc2), (rows, rows2)):
        for x, y in zip(p.to_numpy(), q.to_numpy()):
            assert np.array_equal(x, y)
    if with_tree:
        assert torch.equal(tree.nodes, tree2.nodes) and torch.equal(tree.counts, tree2.counts)
        assert torch.equal(tree.starts, tree2.starts) and tree.n_keys == tree2.n_keys
    return swapped, classes(wr, wch, *want)


def _moves_case(seed):
    """Random replicas with LWW ties everywhere (ts in [-4, 4)); 600 keys of the union: three
    count tiles of the per-key join, the last one partial."""
    rng = np.random.default_rng(seed)
    a, b = W.random_pair(rng, 20_000, n_nodes=5, ts_range=4, dense_ctx=bool(seed % 2))
    kb = np.unique(np.concatenate([a["rows"][0], b["rows"][0]]))
    keys = np.sort(rng.choice(kb, 600, replace=False))
    return a, W.sync_delta(b, keys), keys


@pytest.mark.parametrize("with_tree", [False, True])
@pytest.mark.parametrize("seed", [0, 2])
def test_fused_rows_move(engine, seed, with_tree):
    """The per-key join with rows moving through the spare store.  The inputs must hold every
    class of changed key (on the CPU oracle: 454 and 489 changed keys; unchanged reads 151 /
    190, removed 45 / 31, added 102 / 101, updated 156 / 167, tie-broken winners 53 / 65)."""
    a, d, keys = _moves_case(seed)
    swapped, cls = run(engine, a, d, keys, with_tree=with_tree)
    assert swapped
    assert min(cls.values()) >= 20, cls


def test_fused_in_place(engine):
    """Config-4 shaped: every differing key's one row replaced by one row, in place -- the
    old rows are overwritten, their reads come from the join's own walk."""
    a, b = W.config4_shard(1, 8, keys_per_rank=40_000, diff_frac=0.02)
    want = R.store_diff(a["rows"], b["rows"])
    swapped, cls = run(engine, a, W.sync_delta(b, want), want, depth=12)
    assert not swapped
    assert cls["updated"] + cls["added"] + cls["removed"] > 100


def test_splice_path(monkeypatch):
    """DG_KD=0: the diffs are read from the keyset's taken rows and its edit."""
    monkeypatch.setenv("DG_KD", "0")
    eng = Engine(0)
    try:
        a, d, keys = _moves_case(0)
        swapped, cls = run(eng, a, d, keys)
        assert swapped and min(cls.values()) >= 20
    finally:
        eng.close()


def test_long_key_run(engine):
    """A state key with 70 rows (over the per-key join's 64): the splice serves the call on
    the default engine.  All 70 rows tie on ts, so the smallest value wins; the delta's
    context removes about half of them and its row takes the key over."""
    rng = np.random.default_rng(70)
    keys, a = _runs_state(rng, 3000, 100, 70)
    n = len(a["rows"][0])
    dk = np.sort(np.array([keys[100], keys[5], keys[2000]], np.uint64))
    d = {"rows": (dk, np.array([7, 8, 9], np.uint64), np.full(3, 9, np.int64), np.full(3, 1, np.uint32),
                  np.array([1, 2, 3], np.uint64)),
         "ctx": (R.VV, np.array([0, 1], np.uint32), np.array([n - 35, 3], np.uint64))}
    swapped, cls = run(engine, a, d, dk, depth=9)
    assert swapped and cls["updated"] == 3
    # and with a context that removes nothing: the big key keeps its read on a strictly
    # smaller ts of the delta's row
    d2 = {"rows": d["rows"][:2] + (np.full(3, 2, np.int64),) + d["rows"][3:],
          "ctx": (R.VV, np.array([1], np.uint32), np.array([3], np.uint64))}
    _, cls = run(engine, a, d2, dk, depth=9)
    assert cls["unchanged"] == 3


def test_full_join(engine):
    """Two delta keys outside the keyset: the full join; the diffs are read from the old and
    the joined state."""
    rng = np.random.default_rng(9)
    a, b = W.random_pair(rng, 20_000, n_nodes=4, ts_range=4)
    kb = np.unique(b["rows"][0])
    keys = kb[::100]
    d = W.sync_delta(b, np.union1d(keys, kb[7:9]))
    swapped, cls = run(engine, a, d, keys, with_tree=False)
    assert swapped and cls["updated"] > 0


def _check_read_diff(engine, old, new, keys):
    so, sn = Store.from_numpy(*old, device=DEV), Store.from_numpy(*new, device=DEV)
    got = engine.read_diff(so, sn, kdev(keys))
    for name, x, y in zip(("old_val", "new_val", "flags"), got, expected_diffs(old, new, keys)):
        assert np.array_equal(_np(x), y), name
    return _np(got[2])


def test_read_diff(engine):
    """dg_read_diff alone: keys in any order with repeats -- the changed keys, keys absent from
    both stores, each store's first and last key -- an empty old store, no keys, and a key
    with 200 rows (no run limit)."""
    a, d, keys = _moves_case(0)
    old = a["rows"]
    new, _ = R.join2(old, a["ctx"], d["rows"], d["ctx"], keys=keys)
    rng = np.random.default_rng(5)
    absent = np.setdiff1d(rng.integers(0, 1 << 63, 50, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                          np.concatenate([old[0], new[0]]))
    ends = np.array([old[0][0], old[0][-1], new[0][0], new[0][-1], 0, (1 << 64) - 1], np.uint64)
    ks = rng.permutation(np.concatenate([keys, absent, ends, keys[:40]]))
    fl = _check_read_diff(engine, old, new, ks)
    assert {0, OLD, NEW, OLD | NEW} <= set(fl.tolist())
    none = tuple(c[:0] for c in old)
    assert set(_check_read_diff(engine, none, new, ks).tolist()) == {0, NEW}
    assert _check_read_diff(engine, none, none, ks).max() == 0
    assert engine.read_diff(Store.from_numpy(*old, device=DEV), Store.from_numpy(*new, device=DEV),
                            kdev(np.zeros(0, np.uint64)))[0].numel() == 0
    k200, big = _runs_state(rng, 3000, 100, 200)
    half = tuple(c[::2] for c in big["rows"])  # (still sorted and unique: the key keeps ~100 rows)
    fl = _check_read_diff(engine, big["rows"], half, np.array([k200[100], k200[0], k200[-1], k200[101]], np.uint64))
    assert fl[0] == OLD | NEW


def _host_diffs(engine, cap):
    """A dg_lww_diffs in page-locked host memory (dg_host_alloc) and its three views."""
    p = C.c_void_p()
    _abi.check(engine.lib.dg_host_alloc(engine.h, 17 * cap, C.byref(p)))
    d = _abi.dg_lww_diffs(p.value, p.value + 8 * cap, p.value + 16 * cap, cap)
    ov = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(2 * cap,))
    fl = np.ctypeslib.as_array(C.cast(C.c_void_p(p.value + 16 * cap), C.POINTER(C.c_uint8)), shape=(cap,))
    return p, d, ov[:cap], ov[cap:], fl


def test_host_arrays_equal_device_arrays(engine):
    """The arrays in dg_host_alloc memory: the kernels write them straight to the host."""
    a, d, keys = _moves_case(2)
    st, sc, sd, cd, spare, tree, _ = _setup(engine, a, d, 10, True)
    changed, ov, nv, fl, _ = engine.join_delta_diffs(st, sc, sd, cd, kdev(keys), spare, tree)
    n = changed.numel()
    p, hd, hov, hnv, hfl = _host_diffs(engine, len(keys))
    try:
        st, sc, sd, cd, spare, tree, _ = _setup(engine, a, d, 10, True)
        ch2, x, y, z, _ = engine.join_delta_diffs(st, sc, sd, cd, kdev(keys), spare, tree, diffs=hd)
        assert x is None and y is None and z is None and torch.equal(changed, ch2)
        assert np.array_equal(hov[:n], _np(ov)) and np.array_equal(hnv[:n], _np(nv))
        assert np.array_equal(hfl[:n], _np(fl))
        # dg_read_diff into the same block
        old = Store.from_numpy(*a["rows"], device=DEV)
        so, sn = old.abi(), st.abi()
        _abi.check(engine.lib.dg_read_diff(engine.h, C.byref(so), C.byref(sn),
                                           C.cast(C.c_void_p(changed.data_ptr()), _abi.P64), n, C.byref(hd)))
        assert np.array_equal(hov[:n], _np(ov)) and np.array_equal(hnv[:n], _np(nv))
        assert np.array_equal(hfl[:n], _np(fl))
        hd.cap = n - 1
        assert engine.lib.dg_read_diff(engine.h, C.byref(so), C.byref(sn),
                                       C.cast(C.c_void_p(changed.data_ptr()), _abi.P64), n,
                                       C.byref(hd)) == _abi.DG_E_CAPACITY
    finally:
        engine.lib.dg_host_free(engine.h, p)


def test_capacities_leave_the_state_alone(engine):
    """diffs.cap < cap: DG_E_INVAL; a changed-key buffer too small: DG_E_CAPACITY (the count
    kernel's tree update undone).  Either way the state, its context and the tree are bit
    for bit what they were, and the engine goes on."""
    a, d, keys = _moves_case(0)
    st, sc, sd, cd, spare, tree, _ = _setup(engine, a, d, 10, True)
    snap = _snapshot(st, sc, tree)
    ov, nv, fl, small = engine._diffs(len(keys) - 1)
    with pytest.raises(_abi.DeltaGpuError) as err:
        engine.join_delta_diffs(st, sc, sd, cd, kdev(keys), spare, tree, diffs=small)
    assert err.value.code == _abi.DG_E_INVAL
    _assert_unchanged(st, sc, tree, snap)
    with pytest.raises(_abi.CapacityError):
        engine.join_delta_diffs(st, sc, sd, cd, kdev(keys), spare, tree,
                                changed=torch.empty(5, dtype=torch.int64, device=DEV))
    _assert_unchanged(st, sc, tree, snap)
    run(engine, a, d, keys)


def test_resident_mirror_equals_the_mirror():
    """A term-level history through update_resident_state_with_delta (one state joined in
    place, dg_join_delta_diffs) and through update_state_with_delta (a new state per call):
    the same on_diffs value call for call -- None when nothing changed, `keys` order, a key
    listed twice reported twice, nil read as absent, equal-ts concurrent adds resolved by
    value order -- and the same final read/1."""
    from delta_crdt_ex_amd import aw_lww_map as M
    from delta_crdt_ex_amd import causal_crdt as CC
    a, r = M.compress_dots(M.new()), M.compress_dots(M.new())
    spare = Store.empty(8, M._dev())
    tree = M.merkle_map(r, depth=6)
    seen = []

    def step(delta, keys):
        nonlocal a
        a, want = CC.update_state_with_delta(a, delta, keys)
        got = CC.update_resident_state_with_delta(r, delta, keys, spare, tree)
        assert got == want, (keys, got, want)
        assert M.read(r) == M.read(a)
        seen.append(want)

    step(M.add("Derek", "Kraan", 1, a, ts=10), ["Derek"])
    step(M.add("Derek", "Kraan", 1, a, ts=11), ["Derek"])        # the same value again: []
    step(M.add("Derek", None, 1, a, ts=12), ["Derek"])           # nil: {:remove, "Derek"}
    step(M.remove("Derek", 1, a), ["Derek"])                     # {nil, nil}: []
    step(M.remove("Derek", 1, a), ["Derek"])                     # nothing changed: None
    base = a                                                     # two nodes add concurrently, equal ts
    d1, d2 = M.add("k", "zeta", 1, base, ts=20), M.add("k", "alpha", 2, base, ts=20)
    step(d1, ["k"])
    step(d2, ["k", "Derek", "k"])                                # listed twice: reported twice
    step(M.add("j", 1.0, 2, a, ts=21), ["j", "k"])
    step(M.add("j", 1, 1, a, ts=22), ["k", "j"])                 # 1 =/= 1.0
    step(M.remove("k", 2, a), ["k"])
    assert seen == [[("add", "Derek", "Kraan")], [], [("remove", "Derek")], [], None,
                    [("add", "k", "zeta")], [("add", "k", "alpha"), ("add", "k", "alpha")],
                    [("add", "j", 1.0)], [("add", "j", 1)], [("remove", "k")]]
    assert type(seen[7][0][2]) is float and type(seen[8][0][2]) is int
    fresh = M.merkle_map(r, depth=6)
    assert torch.equal(tree.nodes, fresh.nodes) and tree.n_keys == fresh.n_keys
