"""dg_join_deltas on cuda:0: a batch of deltas joined into a resident state in one call.
The state and its context against the C oracle's delta-by-delta fold (ref.apply_deltas), the
tree against a fresh build of the result, the changed keys against the oracle's diff of the
state before and after (ref.changed_keys / ref.store_diff), the diffs against its two reads.
Engines: the one-pass fold (DG_APPLY_MODE=onepass: it errors instead of stepping) and the
stepwise fold, each with the tree rebuilt (DG_TREE_REBUILD=always) and updated (never)."""
import os

import numpy as np
import pytest
import torch

from delta_crdt_ex_amd._abi import CapacityError
from delta_crdt_ex_amd.store import Engine, Store, u64
from kfold_cases import mutation_fold, random_fold
from lww_diffs_cases import expected_diffs
from oracle import ref as R
from test_gpu_configs import keys_dev
from test_gpu_join_delta import _assert_unchanged, _rows, _snapshot, state_of, up
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu

MODES = [("onepass", "always"), ("onepass", "never"), ("fold", "always"), ("fold", "never")]


@pytest.fixture(scope="module")
def engines():
    made = {}
    for apply_mode, tree_mode in MODES:
        os.environ["DG_APPLY_MODE"], os.environ["DG_TREE_REBUILD"] = apply_mode, tree_mode
        try:
            made[apply_mode, tree_mode] = Engine(0)
        finally:
            del os.environ["DG_APPLY_MODE"], os.environ["DG_TREE_REBUILD"]
    yield made
    for e in made.values():
        e.close()


def _np(t):
    return t.cpu().numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint64)


def setup(eng, st, ds, depth):
    s, c = state_of(st, extra_ctx=sum(len(d["ctx"][1]) for d in ds))
    dd = [up(d) for d in ds]
    ks = [None if d["keys"] is None else keys_dev(d["keys"]) for d in ds]
    total = s.n + sum(x[0].n for x in dd)
    return s, c, dd, ks, Store.empty(total, DEV), eng.merkle_build(s, depth), Store.empty(total, DEV)


def tree_eq(eng, tree, s, depth):
    fresh = eng.merkle_build(s, depth)
    assert torch.equal(tree.nodes, fresh.nodes) and torch.equal(tree.counts, fresh.counts)
    assert torch.equal(tree.starts, fresh.starts) and tree.n_keys == fresh.n_keys


def run(eng, st, ds, depth=10, keyed_only=False):
    """One join_deltas call checked against the oracle; returns the changed keys.
    keyed_only: every delta row's key is in its keyset, so the changed keys are also
    diff/3's over the union of the keysets."""
    s, c, dd, ks, spare, tree, rows = setup(eng, st, ds, depth)
    old_ptr = s.key.data_ptr()
    changed, ov, nv, fl, swapped = eng.join_deltas(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare,
                                                   tree, rows=rows)
    wr, wc = R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds], [d["ctx"] for d in ds],
                            [d["keys"] for d in ds])
    rows_eq(s, wr)
    ctx_eq(c, wc)
    tree_eq(eng, tree, s, depth)
    assert swapped == (len(ds) > 0) and (spare.key.data_ptr() == old_ptr) == swapped
    want = R.store_diff(st["rows"], wr)
    if keyed_only:
        union = np.unique(np.concatenate([d["keys"] for d in ds] + [np.zeros(0, np.uint64)]))
        assert np.array_equal(want, R.changed_keys(st["rows"], wr, union))
    assert np.array_equal(u64(changed), want)
    for name, x, y in zip(("old_val", "new_val", "flags"), (_np(ov), _np(nv), _np(fl)),
                          expected_diffs(st["rows"], wr, want)):
        assert np.array_equal(x, y), name
    m = np.isin(wr[0], want)
    assert rows.n == int(m.sum())
    for x, y in zip(rows.to_numpy(), wr):
        assert np.array_equal(x, y[m])
    return want


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("seed,k", [(0, 1), (1, 3), (3, 17), (4, 64), (5, 65)])
def test_random_folds(engines, mode, seed, k):
    """Sync-shaped batches (p_outside=0: the changed keys are diff/3's) and batches with
    delta rows outside their keysets (carried keys: the store diff's superset)."""
    eng = engines[mode]
    st, ds = random_fold(seed, n_keys=3000, k=k, p_outside=0.0)
    assert len(run(eng, st, ds, keyed_only=True)) > 0
    st, ds = random_fold(seed, n_keys=3000, k=k)
    want = run(eng, st, ds)
    if k >= 3:
        union = np.unique(np.concatenate([d["keys"] for d in ds]))
        assert not np.isin(want, union).all(), "no carried key outside the keysets changed"


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(m))
def test_mutation_deltas(engines, mode):
    """Mutation deltas with dot-set contexts (every row's key in its keyset)."""
    st, ds = mutation_fold(40, n_keys=5000, k=5, ops=200)
    assert all(d["ctx"][0] == 1 for d in ds)
    assert len(run(engines[mode], st, ds, keyed_only=True)) > 0


def _net_case():
    """Key K gets a row from delta 0 that delta 1 removes again (its context covers the new
    dot and K is in its keyset): K's rows are what they were.  Key L is really updated."""
    st, _ = random_fold(7, n_keys=3000, k=0, n_nodes=4)
    keys = np.unique(st["rows"][0])
    K, L = keys[100], keys[2000]
    vv = (R.VV, np.array([900], np.uint32), np.array([2], np.uint64))
    d0 = {"rows": (np.array([K, L], np.uint64), np.array([1 << 62, (1 << 62) + 1], np.uint64),
                   np.array([50, 50], np.int64), np.array([900, 900], np.uint32), np.array([1, 2], np.uint64)),
          "ctx": vv, "keys": np.array(sorted([K, L]), np.uint64)}
    if K > L:
        d0["rows"] = tuple(c[::-1].copy() for c in d0["rows"])
    d1 = {"rows": R.empty_rows(), "ctx": (R.VV, np.array([900], np.uint32), np.array([1], np.uint64)),
          "keys": np.array([K], np.uint64)}
    return st, [d0, d1], K, L


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(m))
def test_net_changes(engines, mode):
    st, ds, K, L = _net_case()
    # (delta by delta, K changes twice)
    mid, mc = R.join2(st["rows"], st["ctx"], ds[0]["rows"], ds[0]["ctx"], ds[0]["keys"])
    end, _ = R.join2(mid, mc, ds[1]["rows"], ds[1]["ctx"], ds[1]["keys"])
    assert K in R.store_diff(st["rows"], mid) and K in R.store_diff(mid, end)
    want = run(engines[mode], st, ds, keyed_only=True)
    assert np.array_equal(want, np.array([L], np.uint64))


def test_resident_mirror_takes_a_batch():
    """Term-level batches through causal_crdt.update_resident_state_with_deltas (one resident
    state, dg_join_deltas) against the same deltas through update_state_with_delta one by one:
    the same final read/1 and tree, and the NET on_diffs value -- each key once, in the order
    of its first occurrence over the batch's key lists, with its final value; a key that
    changes and changes back, and one whose read returns to what it was, report nothing."""
    from delta_crdt_ex_amd import aw_lww_map as M
    from delta_crdt_ex_amd import causal_crdt as CC
    a, r = M.compress_dots(M.new()), M.compress_dots(M.new())
    spare = Store.empty(8, M._dev())
    tree = M.merkle_map(r, depth=6)

    def batch(make):
        """make(state) -> [(delta, keys)], built against the state as the one-by-one replica
        sees it, so both replicas get the same deltas"""
        nonlocal a
        out = []
        for f in make:
            delta, keys = f(a)
            a, _ = CC.update_state_with_delta(a, delta, keys)
            out.append((delta, keys))
        got = CC.update_resident_state_with_deltas(r, out, spare, tree)
        assert M.read(r) == M.read(a)
        fresh = M.merkle_map(r, depth=6)
        assert torch.equal(tree.nodes, fresh.nodes) and tree.n_keys == fresh.n_keys
        return got

    got = batch([lambda s: (M.add("x", 1, 1, s, ts=10), ["x"]),
                 lambda s: (M.add("y", "why", 2, s, ts=11), ["y", "x"]),
                 lambda s: (M.add("x", 2, 1, s, ts=12), ["x"])])
    assert got == [("add", "x", 2), ("add", "y", "why")]          # first occurrence: x, then y
    got = batch([lambda s: (M.add("z", "tmp", 1, s, ts=20), ["z"]),
                 lambda s: (M.remove("z", 1, s), ["z"]),            # z is gone again: nothing
                 lambda s: (M.add("y", None, 2, s, ts=21), ["y"])])  # nil: a remove
    assert got == [("remove", "y")]
    got = batch([lambda s: (M.add("x", 3, 1, s, ts=30), ["x"]),
                 lambda s: (M.add("x", 2, 1, s, ts=31), ["x"])])     # x reads 2 again: changed, no diff
    assert got == []
    assert batch([]) is None                                         # nothing to join: None
    # one delta is the single-delta call
    assert batch([lambda s: (M.add("w", 1.0, 1, s, ts=40), ["w", "w"])]) == [("add", "w", 1.0), ("add", "w", 1.0)]


def test_k0(engine):
    st, _ = random_fold(8, n_keys=3000, k=0)
    s, c, _, _, spare, tree, rows = setup(engine, st, [], 10)
    snap = _snapshot(s, c, tree)
    changed, ov, nv, fl, swapped = engine.join_deltas(s, c, [], [], [], spare, tree, rows=rows)
    assert changed.numel() == 0 and rows.n == 0 and not swapped
    _assert_unchanged(s, c, tree, snap)
    rows_eq(s, st["rows"])


@pytest.mark.parametrize("mode", [("onepass", "always"), ("fold", "never")], ids=lambda m: "-".join(m))
def test_all_or_nothing_capacities(engines, mode):
    """A `changed` one entry too small, and a `spare` one row too small: CapacityError, and
    the state's columns, its context and the tree are bit-equal to before; the next valid
    call gives the oracle's result."""
    eng = engines[mode]
    st, ds = random_fold(9, n_keys=3000, k=6)
    wr, _ = R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds], [d["ctx"] for d in ds],
                           [d["keys"] for d in ds])
    total = len(R.store_diff(st["rows"], wr))
    s, c, dd, ks, spare, tree, rows = setup(eng, st, ds, 10)
    snap = _snapshot(s, c, tree)
    args = ([x[0] for x in dd], [x[1] for x in dd], ks)
    with pytest.raises(CapacityError, match="changed keys"):
        eng.join_deltas(s, c, *args, spare, tree, changed=torch.empty(total - 1, dtype=torch.int64, device=DEV))
    _assert_unchanged(s, c, tree, snap)
    with pytest.raises(CapacityError, match="spare"):
        eng.join_deltas(s, c, *args, Store.empty(s.n + sum(x[0].n for x in dd) - 1, DEV), tree)
    _assert_unchanged(s, c, tree, snap)
    changed, *_ = eng.join_deltas(s, c, *args, spare, tree,
                                  changed=torch.empty(total, dtype=torch.int64, device=DEV))
    assert changed.numel() == total
    rows_eq(s, wr)
    tree_eq(eng, tree, s, 10)


@pytest.mark.parametrize("mode", [("fold", "always"), ("fold", "never")], ids=lambda m: "-".join(m))
def test_failed_tree_step_leaves_the_state_alone(engines, mode):
    """Joined rows that overflow a bucket's 16-bit row count (depth-1 tree, 65530 rows in
    bucket 0, 10 new keys there, in two deltas): DG_E_CAPACITY from the rebuild and from
    the update, and the state, its context and the tree are exactly what they were."""
    eng = engines[mode]
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 1 << 63, 65540, dtype=np.uint64))
    low, e1, e2 = keys[:65530], keys[65530:65535], keys[65535:65540]
    st = {"rows": _rows(low, 0, 1), "ctx": (0, np.array([0], np.uint32), np.array([65530], np.uint64))}
    ds = [{"rows": _rows(e1, 1, 1), "ctx": (0, np.array([1], np.uint32), np.array([5], np.uint64)), "keys": e1},
          {"rows": _rows(e2, 2, 1), "ctx": (0, np.array([2], np.uint32), np.array([5], np.uint64)), "keys": e2}]
    s, c, dd, ks, spare, tree, _ = setup(eng, st, ds, 1)
    snap = _snapshot(s, c, tree)
    with pytest.raises(CapacityError, match="65535"):
        eng.join_deltas(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree)
    _assert_unchanged(s, c, tree, snap)
    run(eng, st, ds, depth=8, keyed_only=True)  # a deeper tree takes the same batch
