"""dg_join_deltas_keyed on cuda:0: a batch of small keyed deltas folded by a thread per key of
the keysets' union.  Every served call is checked against the C oracle's delta-by-delta fold
as test_gpu_join_deltas.run checks dg_join_deltas (rows, context, tree == a fresh build,
changed keys, diffs, the changed keys' rows) and, byte for byte, against Engine.join_deltas
on a second copy of the inputs.  `swapped` is checked against the rule the header states:
rows go through `spare` when a union key's row count changes, or when a key of several rows
loses one and gains one.  Unserved batches return None with nothing touched."""
import numpy as np
import pytest
import torch

import keyed_fold_cases as KC
from delta_crdt_ex_amd._abi import CapacityError, DeltaGpuError
from delta_crdt_ex_amd.store import Store, u64
from kfold_cases import mutation_fold, random_fold
from lww_diffs_cases import expected_diffs
from oracle import ref as R
from test_gpu_configs import keys_dev
from test_gpu_join_delta import _assert_unchanged, _rows, _snapshot, state_of, up
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint64)


def setup(eng, st, ds, depth, shard=(0, 0)):
    s, c = state_of(st, extra_ctx=sum(len(d["ctx"][1]) for d in ds))
    dd = [up(d) for d in ds]
    ks = [None if d["keys"] is None else keys_dev(d["keys"]) for d in ds]
    total = s.n + sum(x[0].n for x in dd)
    tree = eng.merkle_build(s, depth, shard_bits=shard[0], shard=shard[1]) if depth else None
    return s, c, dd, ks, Store.empty(total, DEV), tree, Store.empty(total, DEV)


def oracle(st, ds):
    return R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds], [d["ctx"] for d in ds],
                          [d["keys"] for d in ds])


def rows_move(old, new, union):
    """The header's rule for *swapped, from the oracle's rows."""
    def count(rows):
        return np.searchsorted(rows[0], union, "right") - np.searchsorted(rows[0], union, "left")
    na, ne = count(old), count(new)
    if (na != ne).any():
        return True
    for x in union[na > 1]:
        o, n = set(KC.key_rows(old, x)), set(KC.key_rows(new, x))
        if o - n and n - o:
            return True
    return False


def tree_eq(eng, tree, s, depth, shard):
    fresh = eng.merkle_build(s, depth, shard_bits=shard[0], shard=shard[1])
    assert torch.equal(tree.nodes, fresh.nodes) and torch.equal(tree.counts, fresh.counts)
    assert torch.equal(tree.starts, fresh.starts) and tree.n_keys == fresh.n_keys


def run(eng, st, ds, depth=10, shard=(0, 0), with_rows=True, with_diffs=True, swapped=None):
    """One served join_deltas_keyed call against the oracle and against join_deltas; returns
    (changed keys, swapped).  depth 0: no tree."""
    s, c, dd, ks, spare, tree, rows = setup(eng, st, ds, depth, shard)
    rows = rows if with_rows else None
    old_ptr, spare_before = s.key.data_ptr(), [x.clone() for x in (spare.key, spare.val, spare.ts, spare.node, spare.cnt)]
    got = eng.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree, rows=rows,
                                want_diffs=with_diffs)
    assert got is not None, "the batch was not served"
    changed, ov, nv, fl, sw = got
    wr, wc = oracle(st, ds)
    rows_eq(s, wr)
    ctx_eq(c, wc)
    if tree is not None:
        tree_eq(eng, tree, s, depth, shard)
    union = np.unique(np.concatenate([d["keys"] for d in ds]))
    want_sw = rows_move(st["rows"], wr, union)
    assert sw == want_sw and (spare.key.data_ptr() == old_ptr) == sw
    if swapped is not None:
        assert sw == swapped
    if not sw:  # in place: `spare` was not touched
        for x, y in zip((spare.key, spare.val, spare.ts, spare.node, spare.cnt), spare_before):
            assert torch.equal(x, y)
    want = R.store_diff(st["rows"], wr)
    assert np.array_equal(want, R.changed_keys(st["rows"], wr, union))
    assert np.array_equal(u64(changed), want)
    if with_diffs:
        for name, x, y in zip(("old_val", "new_val", "flags"), (_np(ov), _np(nv), _np(fl)),
                              expected_diffs(st["rows"], wr, want)):
            assert np.array_equal(x, y), name
    m = np.isin(wr[0], want)
    if with_rows:
        assert rows.n == int(m.sum())
        for x, y in zip(rows.to_numpy(), wr):
            assert np.array_equal(x, y[m])
    # ... and byte for byte what dg_join_deltas gives on a second copy of the inputs
    s2, c2, dd2, ks2, spare2, tree2, rows2 = setup(eng, st, ds, depth, shard)
    rows2 = rows2 if with_rows else None
    ch2, ov2, nv2, fl2, _ = eng.join_deltas(s2, c2, [x[0] for x in dd2], [x[1] for x in dd2], ks2, spare2, tree2,
                                            rows=rows2)
    for x, y in zip(s.to_numpy(), s2.to_numpy()):
        assert np.array_equal(x, y)
    for x, y in zip(c.to_numpy(), c2.to_numpy()):
        assert np.array_equal(x, y)
    assert c.kind == c2.kind and torch.equal(changed, ch2)
    if tree is not None:
        assert torch.equal(tree.nodes, tree2.nodes) and torch.equal(tree.counts, tree2.counts)
        assert torch.equal(tree.starts, tree2.starts) and tree.n_keys == tree2.n_keys
    if with_diffs:
        assert torch.equal(ov, ov2) and torch.equal(nv, nv2) and torch.equal(fl, fl2)
    if with_rows:
        assert rows.n == rows2.n
        for x, y in zip(rows.to_numpy(), rows2.to_numpy()):
            assert np.array_equal(x, y)
    return want, sw


def declined(eng, st, ds, depth=10):
    """The call returns None and the state, its context and the tree are what they were."""
    s, c, dd, ks, spare, tree, rows = setup(eng, st, ds, depth)
    snap = _snapshot(s, c, tree)
    got = eng.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree, rows=rows)
    assert got is None
    _assert_unchanged(s, c, tree, snap)


# ---------------------------------------------------------------- served
@pytest.mark.parametrize("seed,k", [(0, 1), (1, 2), (2, 3), (3, 17), (4, 64)])
def test_random_folds(engine, seed, k):
    st, ds = random_fold(seed, n_keys=3000, k=k, p_outside=0.0)
    want, _ = run(engine, st, ds)
    assert len(want) > 0


def test_ten_count_workgroups(engine):
    """A 20,000-key state and 64 deltas of 40 keys: 2,560 union keys, ten count workgroups."""
    st, _ = random_fold(11, n_keys=20_000, k=0)
    keys = np.unique(st["rows"][0])
    _, pool = random_fold(12, n_keys=20_000, k=1, p_keys=1.0, p_outside=0.0)  # rows of every key to draw from
    prow = pool[0]["rows"]
    rng = np.random.default_rng(13)
    pick = rng.permutation(keys)[:2560].reshape(64, 40)
    ds = []
    for i in range(64):
        ki = np.sort(pick[i])
        m = np.isin(prow[0], ki)
        ds.append({"rows": tuple(c[m] for c in prow), "ctx": pool[0]["ctx"], "keys": ki})
    assert len(np.unique(np.concatenate([d["keys"] for d in ds]))) == 2560
    want, _ = run(engine, st, ds, depth=12)
    assert len(want) > 256


def test_count_workgroups_past_one_round(engine):
    """A state of about 70,000 keys and 64 deltas of 1,025 disjoint keys: 65,600 union keys, 257
    count workgroups -- the fewest for which the last workgroup's sum over the workgroups'
    figures (256 per round) takes a second round."""
    st, _ = random_fold(15, n_keys=90_000, k=0)
    keys = np.unique(st["rows"][0])
    assert 65_600 < len(keys) < 75_000
    _, pool = random_fold(16, n_keys=90_000, k=1, p_keys=1.0, p_outside=0.0)  # rows of every key to draw from
    prow = pool[0]["rows"]
    rng = np.random.default_rng(17)
    pick = rng.permutation(keys)[:65_600].reshape(64, 1025)
    ds = []
    for i in range(64):
        ki = np.sort(pick[i])
        m = np.isin(prow[0], ki)
        ds.append({"rows": tuple(c[m] for c in prow), "ctx": pool[0]["ctx"], "keys": ki})
    assert len(np.unique(np.concatenate([d["keys"] for d in ds]))) == 65_600 == 256 * 256 + 64
    want, _ = run(engine, st, ds, depth=14)
    assert len(want) > 10_000


def test_union_through_the_sort(engine):
    """64 keysets of about 600 keys: 38,000 items, past the total at which the union ranks the
    items in the keysets (items x keysets <= 2^21) and so through the radix sort."""
    st, ds = random_fold(14, n_keys=20_000, k=64, p_keys=0.03, p_outside=0.0)
    assert sum(len(d["keys"]) for d in ds) * 64 > 1 << 21
    want, _ = run(engine, st, ds, depth=12)
    assert len(want) > 1000


def test_unsorted_keyset_through_the_sort(engine):
    st, ds = random_fold(14, n_keys=20_000, k=64, p_keys=0.03, p_outside=0.0)
    s, c, dd, ks, spare, tree, _ = setup(engine, st, ds, 10)
    ks[5] = ks[5].flip(0).contiguous()
    snap = _snapshot(s, c, tree)
    with pytest.raises(DeltaGpuError, match="ascending"):
        engine.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree)
    _assert_unchanged(s, c, tree, snap)


@pytest.mark.parametrize("n_union", [255, 256, 257])
def test_union_sizes_at_the_workgroup_seam(engine, n_union):
    st, keys = KC.base()
    cut = n_union // 3
    ds = [KC.delta([(int(keys[5]), KC.V0, 99, 900, 1)], {900: 1}, keys[:2 * cut]),
          KC.delta([(int(keys[n_union - 1]), KC.V0, 99, 901, 1)], {901: 1}, keys[cut:n_union])]
    assert len(np.unique(np.concatenate([d["keys"] for d in ds]))) == n_union
    want, _ = run(engine, st, ds)
    assert len(want) == 2


def test_net_no_change(engine):
    st, ds, K, L = KC.net_no_change()
    want, _ = run(engine, st, ds)
    assert np.array_equal(want, np.array([L], np.uint64))


def test_order_dependence(engine):
    st, ds, x, r = KC.order_dependence()
    run(engine, st, ds)


def test_remove_then_readd(engine):
    st, ds, x, old, fresh = KC.remove_then_readd()
    want, _ = run(engine, st, ds)
    assert np.uint64(x) in want


def test_shared_tuple(engine):
    st, ds, tuples = KC.shared_tuple()
    want, _ = run(engine, st, ds)
    assert len(want) == 3


def test_empty_key(engine):
    st, ds, z, L = KC.empty_key()
    want, _ = run(engine, st, ds)
    assert np.array_equal(want, np.array([L], np.uint64))


def test_hazard_goes_through_spare(engine):
    st, ds, h, want_rows = KC.hazard()
    want, sw = run(engine, st, ds, swapped=True)
    assert np.array_equal(want, np.array([h], np.uint64))


@pytest.mark.parametrize("n_state,n_cand", [(64, 2), (3, 64)])
def test_row_limits_served(engine, n_state, n_cand):
    st, ds, b = KC.row_limits(n_state, n_cand)
    want, _ = run(engine, st, ds)
    assert np.array_equal(want, np.array([b], np.uint64))


def test_rows_in_one_delta(engine):
    """64 rows of a key in one delta are served, 65 are declined (the per-delta limit)."""
    st, ds, b = KC.rows_in_one_delta(64)
    want, _ = run(engine, st, ds)
    assert np.array_equal(want, np.array([b], np.uint64))
    declined(engine, *KC.rows_in_one_delta(65)[:2])


def _in_place_batch():
    """Every key keeps its count and no key of several rows changes: one-row keys get their
    row replaced, other keys are named and untouched."""
    st, keys = KC.base()
    rows = st["rows"]
    single = [int(k) for k in keys[:400] if (rows[0] == k).sum() == 1][:40]
    assert len(single) == 40
    ds = []
    for i in range(4):
        mine = single[i * 10:(i + 1) * 10]
        cover = {}
        for x in mine:
            r = KC.key_rows(rows, x)[0]
            cover[r[3]] = max(cover.get(r[3], 0), r[4])
        # (the VV also covers other keys' dots: only single-row keys and absent keys are named)
        new = [(x, KC.V0 + 7, 100 + i, 920 + i, j + 1) for j, x in enumerate(mine)]
        ds.append(KC.delta(new, {**cover, 920 + i: 10}, mine))
    return st, ds


def test_in_place(engine):
    st, ds = _in_place_batch()
    want, sw = run(engine, st, ds, swapped=False)
    assert len(want) == 40


def test_new_keys_and_deleted_keys(engine):
    st, keys = KC.base()
    gone = [int(k) for k in keys[300:330]]
    cover = {n: 1 << 40 for n in range(4)}
    new = [(KC.absent_key(keys, 10 + i), KC.V0, 5, 930, i + 1) for i in range(30)]
    ds = [KC.delta([], cover, gone), KC.delta(new, {930: 30}, [t[0] for t in new])]
    want, sw = run(engine, st, ds, swapped=True)
    assert len(want) == 60


def test_shard_tree(engine):
    st, ds = random_fold(21, n_keys=3000, k=5, p_outside=0.0)
    sh = lambda k: (np.asarray(k, np.uint64) >> np.uint64(62)) == 1  # noqa: E731  (shard 1 of 4)
    st = {**st, "rows": tuple(c[sh(st["rows"][0])] for c in st["rows"])}
    ds = [{"rows": tuple(c[sh(d["rows"][0])] for c in d["rows"]), "ctx": d["ctx"], "keys": d["keys"][sh(d["keys"])]}
          for d in ds]
    want, _ = run(engine, st, ds, depth=9, shard=(2, 1))
    assert len(want) > 0


@pytest.mark.parametrize("what", ["tree", "rows", "diffs"])
def test_without(engine, what):
    st, ds = random_fold(22, n_keys=3000, k=4, p_outside=0.0)
    run(engine, st, ds, depth=0 if what == "tree" else 10, with_rows=what != "rows", with_diffs=what != "diffs")


def test_mutation_deltas_fall_back(engine):
    """Mutation deltas carry dot-set contexts: the header promises DG_KEYED_FALLBACK."""
    st, ds = mutation_fold(40, n_keys=5000, k=5, ops=200)
    assert all(d["ctx"][0] == 1 for d in ds)
    declined(engine, st, ds)


# ---------------------------------------------------------------- fallbacks
def test_row_outside_its_keyset(engine):
    st, ds = random_fold(3, n_keys=3000, k=17)
    assert not all(np.isin(d["rows"][0], d["keys"]).all() for d in ds)
    declined(engine, st, ds)


def test_null_keyset(engine):
    st, ds = random_fold(5, n_keys=3000, k=4, p_outside=0.0)
    ds[2]["keys"] = None
    declined(engine, st, ds)


def test_k65(engine):
    st, ds = random_fold(5, n_keys=3000, k=65, p_outside=0.0)
    declined(engine, st, ds)


def test_node_id_past_the_tables(engine):
    st, ds = random_fold(6, n_keys=3000, k=4, p_outside=0.0)
    kind, node, cnt = ds[1]["ctx"]
    ds[1]["ctx"] = (kind, np.append(node, np.uint32(1024)), np.append(cnt, np.uint64(3)))
    declined(engine, st, ds)


def test_dot_set_state_context(engine):
    st, ds = random_fold(6, n_keys=3000, k=4, p_outside=0.0, dots_ctx=True)
    assert st["ctx"][0] == 1
    declined(engine, st, ds)


@pytest.mark.parametrize("n_state,n_cand", [(65, 2), (3, 65)])
def test_row_limits_fall_back(engine, n_state, n_cand):
    st, ds, b = KC.row_limits(n_state, n_cand)
    declined(engine, st, ds)


# ---------------------------------------------------------------- all or nothing
def test_all_or_nothing_capacities(engine):
    st, ds = random_fold(9, n_keys=3000, k=6, p_outside=0.0)
    wr, _ = oracle(st, ds)
    total = len(R.store_diff(st["rows"], wr))
    s, c, dd, ks, spare, tree, rows = setup(engine, st, ds, 10)
    snap = _snapshot(s, c, tree)
    args = ([x[0] for x in dd], [x[1] for x in dd], ks)
    with pytest.raises(CapacityError, match="changed keys"):
        engine.join_deltas_keyed(s, c, *args, spare, tree,
                                 changed=torch.empty(total - 1, dtype=torch.int64, device=DEV))
    _assert_unchanged(s, c, tree, snap)
    with pytest.raises(CapacityError, match="spare"):
        engine.join_deltas_keyed(s, c, *args, Store.empty(s.n + sum(x[0].n for x in dd) - 1, DEV), tree)
    _assert_unchanged(s, c, tree, snap)
    changed, *_ = engine.join_deltas_keyed(s, c, *args, spare, tree,
                                           changed=torch.empty(total, dtype=torch.int64, device=DEV))
    assert changed.numel() == total
    rows_eq(s, wr)
    tree_eq(engine, tree, s, 10, (0, 0))


def test_failed_tree_step_leaves_the_state_alone(engine):
    """test_gpu_join_deltas' overflow of a bucket's 16-bit row count, through the keyed call."""
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 1 << 63, 65540, dtype=np.uint64))
    low, e1, e2 = keys[:65530], keys[65530:65535], keys[65535:65540]
    st = {"rows": _rows(low, 0, 1), "ctx": (0, np.array([0], np.uint32), np.array([65530], np.uint64))}
    ds = [{"rows": _rows(e1, 1, 1), "ctx": (0, np.array([1], np.uint32), np.array([5], np.uint64)), "keys": e1},
          {"rows": _rows(e2, 2, 1), "ctx": (0, np.array([2], np.uint32), np.array([5], np.uint64)), "keys": e2}]
    s, c, dd, ks, spare, tree, _ = setup(engine, st, ds, 1)
    snap = _snapshot(s, c, tree)
    with pytest.raises(CapacityError, match="65535"):
        engine.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree)
    _assert_unchanged(s, c, tree, snap)
    run(engine, st, ds, depth=8)  # a deeper tree takes the same batch


def test_unsorted_keyset_is_an_error(engine):
    st, ds = random_fold(5, n_keys=3000, k=3, p_outside=0.0)
    s, c, dd, ks, spare, tree, _ = setup(engine, st, ds, 10)
    ks[1] = ks[1].flip(0).contiguous()
    snap = _snapshot(s, c, tree)
    with pytest.raises(DeltaGpuError, match="ascending"):
        engine.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree)
    _assert_unchanged(s, c, tree, snap)


# ---------------------------------------------------------------- interleaving
def test_interleaved_with_the_other_joins(engine):
    """keyed, join_delta, join_deltas and keyed again on one engine and one state: the count
    block, the arrival words and the scratch are shared."""
    st, _ = random_fold(30, n_keys=3000, k=0)
    batches = [random_fold(31 + i, n_keys=3000, k=3, p_outside=0.0)[1] for i in range(4)]
    s, c = state_of(st, extra_ctx=sum(len(d["ctx"][1]) for b in batches for d in b))
    tree = engine.merkle_build(s, 10)
    rows, ctx = st["rows"], st["ctx"]
    for step, ds in enumerate(batches):
        dd = [up(d) for d in ds]
        ks = [keys_dev(d["keys"]) for d in ds]
        spare = Store.empty(s.n + sum(x[0].n for x in dd), DEV)
        if step in (0, 3):
            assert engine.join_deltas_keyed(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree) is not None
        elif step == 1:
            for (sd, cd), kk in zip(dd, ks):
                engine.join_delta(s, c, sd, cd, kk, Store.empty(s.n + sd.n, DEV), tree)
        else:
            engine.join_deltas(s, c, [x[0] for x in dd], [x[1] for x in dd], ks, spare, tree)
        rows, ctx = R.apply_deltas(rows, ctx, [d["rows"] for d in ds], [d["ctx"] for d in ds], [d["keys"] for d in ds])
        rows_eq(s, rows)
        ctx_eq(c, ctx)
        tree_eq(engine, tree, s, 10, (0, 0))
