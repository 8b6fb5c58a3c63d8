"""dg_replace_keysets (Engine.replace_keysets): k journal records applied to a resident state
as one splice, checked bit for bit against storage.replay_arrays (the host restatement: the
last record naming a key wins) and, for the tree, against a fresh dg_merkle_build of the result.

Shapes: a state of about 10,000 rows -- five splice tiles of 2,048 rows (csrc/splice.hip), keys
of 1 to 5 rows, a run straddling a tile seam and in the union -- and a union of about 1,500
keys: past the 256-key take tile, the 512-key home path and one 1,024-item union tile
(csrc/replay.hip).  k = 1, 3, 70 and 300 records: past one u64 of set bits, so nothing can have
gone through the 64-keyset masks.  The error inputs are rejected by host-side checks or by the
input-error word before anything is written; no case provokes a device fault."""
import numpy as np
import pytest
import torch

import journal_cases as J
from delta_crdt_ex_amd import _abi, storage
from delta_crdt_ex_amd.store import Store

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLICE_TILE = 2048  # csrc/dg_launch.h
TOP = np.uint64(1) << np.uint64(63)


def _kt(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64).copy()).to(DEV)


def _rows_with_counts(rng, keys, counts, node, counter):
    """Exactly counts[i] rows of keys[i], fresh dots of `node`."""
    ks = np.repeat(np.asarray(keys, np.uint64), counts)
    n = len(ks)
    rows = J.sort_rows(ks, rng.integers(0, 1 << 20, n).astype(np.uint64) + np.uint64(1 << 62),
                       rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), np.full(n, node, np.uint32),
                       np.arange(counter, counter + n, dtype=np.uint64))
    return rows, counter + n


class Case:
    """The key space (4,000 hashed ids; `shard`: the top bit clear, for a 1-bit shard tree), the
    state on its keys 100..3369 with 1..5 rows each, and the pool of 1,500 union keys: 50 below
    the first state key, 50 above the last, 1,400 of the state's, a seam-straddling one among
    them."""

    def __init__(self, shard):
        self.rng = np.random.default_rng(77)
        space = J.key_space(4000, 21)
        if shard:
            space = np.unique(space & ~TOP)
        self.space = space
        self.skeys = space[100:3370]
        self.rows, self.counter = J.rows_for(self.rng, self.skeys, 0, 1, lo=1, hi=5)
        k = self.rows[0]
        assert 9000 < len(k) <= 5 * SPLICE_TILE and len(k) > 4 * SPLICE_TILE  # five tiles
        seams = [i for i in range(SPLICE_TILE, len(k), SPLICE_TILE) if k[i - 1] == k[i]]
        assert seams, "no run straddles a tile seam"
        self.seam_key = k[seams[0]]
        inner = np.setdiff1d(self.skeys, [self.seam_key])
        self.pool = np.sort(np.concatenate([space[:50], space[-50:], [self.seam_key],
                                            self.rng.choice(inner, 1399, replace=False)]))
        assert self.pool[0] < self.skeys[0] and self.pool[-1] > self.skeys[-1]
        self.counts = dict(zip(*[x.tolist() for x in np.unique(k, return_counts=True)]))

    def records(self, k, seed, keep_counts=False, grow=None):
        """k records over the pool.  Every pool key is named by at least one record and about
        a third by several; with k >= 3 one key goes add -> remove -> add and another's last
        record removes it; with k >= 4 record 1 has no keys.  keep_counts: every record gives each of its keys
        exactly the rows the state holds of it (only state keys are named), so nothing moves;
        grow: but this key gets one row more."""
        rng = np.random.default_rng(seed)
        pool = np.intersect1d(self.pool, self.skeys) if keep_counts else self.pool
        owner = rng.integers(0, k, len(pool))
        extra_k = rng.choice(pool, len(pool) // 3, replace=False)
        extra_o = rng.integers(0, k, len(extra_k))
        sets = [np.union1d(pool[owner == j], extra_k[extra_o == j]) for j in range(k)]
        a, b = pool[7], pool[11]  # a: add, remove, add again; b: removed by its last record
        forced = {}
        if k >= 3:
            if k >= 4:
                sets[0] = np.union1d(sets[0], sets[1])
                sets[1] = np.zeros(0, np.uint64)
            if not keep_counts:
                sets = [np.setdiff1d(s, [a, b]) for s in sets]
                for j, how in ((0, "add"), (1 if k == 3 else k // 2, "remove"), (k - 1, "add")):
                    sets[j] = np.union1d(sets[j], [a])
                    forced[(j, a)] = how
                sets[0] = np.union1d(sets[0], [b])
                sets[k - 1] = np.union1d(sets[k - 1], [b])
                forced[(0, b)], forced[(k - 1, b)] = "add", "remove"
        recs, counter = [], self.counter
        for j, ks in enumerate(sets):
            ks = ks.astype(np.uint64)
            if keep_counts:
                cnt = np.array([self.counts[x] + (1 if grow is not None and x == grow else 0)
                                for x in ks.tolist()], np.int64)
            else:
                cnt = np.where(rng.random(len(ks)) < 0.25, 0, rng.integers(1, 6, len(ks)))
                for i, x in enumerate(ks.tolist()):
                    how = forced.get((j, x))
                    if how:
                        cnt[i] = 0 if how == "remove" else max(cnt[i], 1)
            rows, counter = _rows_with_counts(rng, ks, cnt, 1 + j % 5, counter)
            recs.append(J.record(ks, rows))
        assert np.array_equal(np.unique(np.concatenate([r["keys"] for r in recs])), pool)
        return recs


@pytest.fixture(scope="module", params=["full", "shard"])
def case(request):
    return Case(request.param == "shard")


@pytest.fixture(scope="module")
def shard_case():
    return Case(True)


def _tree(engine, s, case_shard):
    return engine.merkle_build(s, 10, shard_bits=1 if case_shard else 0, shard=0)


def _is_shard(c):
    return not bool((c.space & TOP).any())


def _apply(engine, c, state_rows, recs, with_tree=True):
    """Upload, replace, compare with replay_arrays and (tree) a fresh build.  Returns swapped."""
    state = Store.from_numpy(*state_rows, device=DEV)
    n_rec_rows = sum(len(r["rows"][0]) for r in recs)
    spare = Store.empty(len(state_rows[0]) + n_rec_rows, DEV)
    tree = _tree(engine, state, _is_shard(c)) if with_tree else None
    keysets = [_kt(r["keys"]) for r in recs]
    stores = [Store.from_numpy(*r["rows"], device=DEV) for r in recs]
    n_union, swapped = engine.replace_keysets(state, keysets, stores, spare, tree)
    want = storage.replay_arrays(state_rows, recs)
    got = state.to_numpy()
    assert state.n == len(want[0])
    for name, x, y in zip(("key", "val", "ts", "node", "cnt"), got, want):
        assert np.array_equal(x, y), name
    all_keys = np.concatenate([r["keys"] for r in recs]) if recs else np.zeros(0, np.uint64)
    assert n_union == len(np.unique(all_keys))
    if with_tree:
        fresh = _tree(engine, Store.from_numpy(*want, device=DEV), _is_shard(c))
        assert torch.equal(tree.nodes, fresh.nodes)
        assert np.array_equal(tree.bucket_counts(), fresh.bucket_counts())
        assert tree.n_keys == fresh.n_keys == len(np.unique(want[0])) and tree.store is state
    return swapped, want


@pytest.mark.parametrize("k", [1, 3, 70, 300])
def test_replace_matches_the_host_replay(engine, case, k):
    recs = case.records(k, seed=k)
    swapped, want = _apply(engine, case, case.rows, recs)
    assert swapped  # removed and added keys: rows moved
    if k >= 3:
        a, b = case.pool[7], case.pool[11]
        assert k == 3 or len(recs[1]["keys"]) == 0  # the record with no keys
        mid = recs[1 if k == 3 else k // 2]
        assert a in mid["keys"] and a not in mid["rows"][0] and a in recs[0]["rows"][0]  # add, remove,
        last_a = recs[k - 1]["rows"]                                                     # add again
        assert np.array_equal(want[4][want[0] == a], last_a[4][last_a[0] == a]) and (want[0] == a).any()
        assert not (want[0] == b).any()  # removed by the last record naming it
    assert (want[0] < case.skeys[0]).any() and (want[0] > case.skeys[-1]).any()  # keys beyond both ends
    named = np.concatenate([r["keys"] for r in recs])
    assert case.seam_key in named and len(named) > 1024 and len(np.unique(named)) == 1500
    if k > 1:  # several records wrote one key, and the last one's rows are the state's
        ks, n = np.unique(named, return_counts=True)
        assert (n > 1).sum() > 100


@pytest.mark.parametrize("k", [3, 70])
def test_empty_state(engine, case, k):
    swapped, want = _apply(engine, case, J.empty_rows(), case.records(k, seed=5))
    assert swapped and len(want[0]) > 1000


@pytest.mark.parametrize("k", [1, 70])
def test_equal_row_counts_stay_in_place(engine, case, k):
    recs = case.records(k, seed=9, keep_counts=True)
    swapped, want = _apply(engine, case, case.rows, recs)
    assert not swapped and len(want[0]) == len(case.rows[0]) and not J.rows_equal(want, case.rows)


def test_one_changed_count_goes_through_spare(engine, case):
    grow = np.intersect1d(case.pool, case.skeys)[700]
    recs = case.records(70, seed=9, keep_counts=True, grow=grow)
    swapped, want = _apply(engine, case, case.rows, recs)
    assert swapped and len(want[0]) == len(case.rows[0]) + 1


def test_more_taken_rows_than_the_first_guess(engine, case):
    """The take of the union's state rows is sized by a guess, 16 rows a key + 4,096
    (api_replay.hip); 10 keys of 450 rows each are past it (4,500 > 4,256), so the call takes
    again at the count the first take reported."""
    rng = np.random.default_rng(12)
    keys = case.space[200:212]
    rows, counter = _rows_with_counts(rng, keys, [450] * 12, 0, 1)
    r0, counter = _rows_with_counts(rng, keys[:6], [2, 0, 450, 1, 451, 3], 1, counter)
    r1, counter = _rows_with_counts(rng, keys[4:10], [5, 0, 2, 0, 1, 7], 2, counter)
    swapped, want = _apply(engine, case, rows, [J.record(keys[:6], r0), J.record(keys[4:10], r1)])
    assert swapped and len(want[0]) == 2 + 450 + 1 + 5 + 2 + 1 + 7 + 2 * 450


def test_without_a_tree(engine, case):
    swapped, _ = _apply(engine, case, case.rows, case.records(3, seed=2), with_tree=False)
    assert swapped


def test_no_records_and_empty_union_are_no_ops(engine, case):
    for recs in ([], [J.record([], J.empty_rows()), J.record([], J.empty_rows())]):
        swapped, want = _apply(engine, case, case.rows, recs)
        assert not swapped and J.rows_equal(want, case.rows)


def _snapshot(state, spare, tree):
    cols = [getattr(s, f).clone() for s in (state, spare) for f in ("key", "val", "ts", "node", "cnt")]
    return cols + [tree.nodes.clone(), tree.counts.clone()], (state.n, spare.n, tree.n_keys)


@pytest.mark.parametrize("what", ["unsorted keyset", "row outside its keyset", "key outside the shard",
                                  "short spare"])
def test_error_inputs_touch_nothing(engine, shard_case, what):
    case = shard_case  # (a 1-bit shard tree: a key can lie outside it)
    recs = case.records(3, seed=4)
    ks, rows = recs[2]["keys"].copy(), recs[2]["rows"]
    code, match = _abi.DG_E_INVAL, None
    if what == "unsorted keyset":
        ks[[5, 6]] = ks[[6, 5]]
        code, match = _abi.DG_E_ORDER, "strictly ascending"
    elif what == "row outside its keyset":
        stray = rows[0][len(rows[0]) // 2]
        ks = ks[ks != stray]
        match = "not in its record's keyset"
    elif what == "key outside the shard":
        out_key = np.uint64(case.pool[-1]) | TOP
        extra, _ = _rows_with_counts(np.random.default_rng(1), [out_key], [2], 9, 1 << 40)
        ks = np.append(ks, out_key)
        rows = tuple(np.concatenate([a, b]) for a, b in zip(rows, extra))
        match = "outside the tree's shard"
    recs[2] = J.record(ks, rows)
    state = Store.from_numpy(*case.rows, device=DEV)
    n_rec_rows = sum(len(r["rows"][0]) for r in recs)
    spare = Store.empty(state.n + n_rec_rows - (1 if what == "short spare" else 0), DEV)
    for f in ("key", "val", "ts", "node", "cnt"):
        getattr(spare, f).fill_(0x5A)
    tree = _tree(engine, state, _is_shard(case))
    before, counts = _snapshot(state, spare, tree)
    with pytest.raises(_abi.DeltaGpuError, match=match) as ei:
        engine.replace_keysets(state, [_kt(r["keys"]) for r in recs],
                               [Store.from_numpy(*r["rows"], device=DEV) for r in recs], spare, tree)
    assert ei.value.code == (_abi.DG_E_CAPACITY if what == "short spare" else code)
    after, counts2 = _snapshot(state, spare, tree)
    assert counts == counts2
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    # and the engine serves the next call
    _apply(engine, case, case.rows, case.records(3, seed=4))
