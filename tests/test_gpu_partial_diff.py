"""The partial Merkle diff (csrc/merkle_cont.hip: dg_merkle_prepare / dg_merkle_continue /
dg_merkle_truncate and the one-workgroup dg_merkle_continue_home) on the inputs hashed
one-row-per-key replicas never make (tests/partial_diff_cases.py): buckets of 0..33 rows
around the register path's 8 | 16 | 17 steps, keys that own several rows, keys and whole
buckets on one side only, an empty store, keys 0 and 2^64 - 1, small shard trees, more
than 512 differing buckets, skewed key sets, a 20,000-row key, term-hash trees.  Every hop
is compared with the C oracle's (oracle/ref.py), bit for bit; the keys a run ends in are
the exact row-set diff (R.store_diff), or its keys in the buckets the truncations kept."""
import os
import random
import sys

import numpy as np
import pytest

import partial_diff_cases as P
import skew
from delta_crdt_ex_amd._abi import DeltaGpuError
from delta_crdt_ex_amd.interning import Universe
from delta_crdt_ex_amd.store import MerkleCont, Store, u64
from oracle import ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["general", "home"]
_CACHE: dict = {}


def side(engine, rows, depth, shard_bits=0, shard=0):
    """(device tree, oracle tree, rows) of one replica; the built tree and its row counts
    are checked against the oracle's once, then shared by the tests."""
    key = (tuple(id(c) for c in rows), depth, shard_bits, shard)  # (the cache keeps the arrays alive)
    if key not in _CACHE:
        s = Store.from_numpy(*rows, device=DEV)
        t = engine.merkle_build(s, depth, shard_bits=shard_bits, shard=shard)
        r = R.merkle_build(rows, depth, shard_bits, shard)
        assert t.n_keys == r.n_keys
        assert np.array_equal(u64(t.nodes), r.nodes)
        assert np.array_equal(t.bucket_counts(), r.counts)
        _CACHE[key] = (t, r, rows)
    return _CACHE[key]


def check_keys(out, full, tree, max_sync):
    if max_sync is None:
        assert np.array_equal(out["keys"], full)
    else:
        assert np.array_equal(out["keys"], P.kept_keys(full, tree, out["kept"]))


# ---------------------------------------------------------------- the ladder
@pytest.mark.parametrize("b_prepares", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("max_sync", [None, 5, 1])
@pytest.mark.parametrize("levels", [8, 3, 1])
@pytest.mark.parametrize("shard_bits,shard", [(0, 0), (2, 1), (2, 3)])
def test_ladder(engine, shard_bits, shard, levels, max_sync, mode, b_prepares):
    a, b, _ = P.ladder(8, shard_bits, shard)
    sa, sb = side(engine, a, 8, shard_bits, shard), side(engine, b, 8, shard_bits, shard)
    first, second = (sb, sa) if b_prepares else (sa, sb)
    out = P.run_protocol(first, second, levels, max_sync, mode, engine)
    check_keys(out, R.store_diff(a, b), sa[1], max_sync)
    if mode == "home":
        assert out["homed"] == out["hops"]  # never declined (test_partial_diff_cases.py)


@pytest.mark.parametrize("empty_prepares", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("levels", [8, 3])
def test_ladder_against_an_empty_store(engine, levels, mode, empty_prepares):
    a, _, _ = P.ladder(8)
    if "empty" not in _CACHE:
        _CACHE["empty"] = P.empty_rows()
    sa, se = side(engine, a, 8), side(engine, _CACHE["empty"], 8)
    first, second = (se, sa) if empty_prepares else (sa, se)
    out = P.run_protocol(first, second, levels, None, mode, engine)
    assert np.array_equal(out["keys"], np.unique(a[0]))
    if mode == "home":
        assert out["homed"] == out["hops"]


@pytest.mark.parametrize("cap", [1, 7])
def test_cap_below_the_result(engine, cap):
    """The leaf-form hop with room for fewer keys than differ: the first `cap` of them, and
    the whole count."""
    a, b, _ = P.ladder(8)
    sa, sb = side(engine, a, 8), side(engine, b, 8)
    full = R.store_diff(a, b)
    leaf = engine.merkle_continue(sb[0], engine.merkle_prepare(sa[0], 8), 8)[1]
    assert leaf.leaf and leaf.n <= P.HOME_ENTRIES and leaf.n_buckets <= P.HOME_BUCKETS
    for res in (engine.merkle_continue(sa[0], leaf, 8, cap=cap),
                engine.merkle_continue_home(sa[0], leaf, 8, None, cap=cap)):
        assert res[0] == "ok" and res[2] == len(full) > 7
        assert np.array_equal(u64(res[1]), full[:cap])


def test_leaf_form_bucket_outside_the_tree(engine):
    a, b, _ = P.ladder(8)
    sa, sb = side(engine, a, 8), side(engine, b, 8)
    leaf = engine.merkle_continue(sb[0], engine.merkle_prepare(sa[0], 8), 8)[1]
    assert leaf.leaf and leaf.n_buckets > 3
    bad = MerkleCont(leaf.level, leaf.pos, leaf.hash, leaf.n, leaf.bucket.clone(), leaf.n_buckets)
    bad.bucket[3] = 1 << 8
    with pytest.raises(DeltaGpuError, match="outside the tree"):
        engine.merkle_continue_home(sa[0], bad, 8, None)
    # a validated input error: the engine goes on, and the correct hop gives the keys
    res = engine.merkle_continue_home(sa[0], leaf, 8, None)
    assert res[0] == "ok" and np.array_equal(u64(res[1]), R.store_diff(a, b))


# ---------------------------------------------------------------- more than 512 differing buckets
@pytest.mark.parametrize("max_sync,n_buckets", [(None, 1448), (600, 600)])
def test_wide_pair_bucket_level(engine, max_sync, n_buckets):
    """Depth 11, levels 11: the prepared continuation is the 2048 buckets themselves, and the
    home path's reply lists more buckets than it has threads (8 per thread over global
    memory).  It equals the oracle's and the general path's; the leaf form is then over the
    home limits, and the general path ends the run."""
    a, b = P.wide_pair()
    sa, sb = side(engine, a, 11), side(engine, b, 11)
    cont = engine.merkle_prepare(sa[0], 11)
    assert cont.n == 2048
    got = engine.merkle_continue_home(sb[0], cont, 11, max_sync)
    want = engine.merkle_continue(sb[0], cont, 11)
    rc = R.merkle_continue(sb[1], b, R.merkle_prepare(sa[1], 11), 11)[1]
    if max_sync is not None:
        engine.merkle_truncate(sb[0], want[1], max_sync)
        rc = R.merkle_truncate(sb[1], rc, max_sync)
    assert got[0] == want[0] == "continue"
    assert len(rc[1]) == n_buckets > P.HOME_BUCKETS
    P.assert_cont_equals(got[1], rc, 11)
    P.assert_cont_equals(want[1], rc, 11)
    assert engine.merkle_continue_home(sa[0], got[1], 11, max_sync) == ("declined",)
    out = P.run_protocol(sa, sb, 11, max_sync, "home", engine)
    assert out["homed"] == 1 and out["hops"] == 2
    check_keys(out, R.store_diff(a, b), sa[1], max_sync)


def test_wide_pair_exactly_the_entry_limit(engine):
    """Depth 12, levels 12: 4096 entries, exactly the home path's limit, are accepted."""
    a, b = P.wide_pair()
    sa, sb = side(engine, a, 12), side(engine, b, 12)
    for first, second in ((sa, sb), (sb, sa)):
        out = P.run_protocol(first, second, 12, None, "home", engine)
        assert out["sizes"][0][1] == 1900 and out["homed"] == 1 and out["hops"] == 2
        assert np.array_equal(out["keys"], R.store_diff(a, b))


# ---------------------------------------------------------------- skewed key sets
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("levels,max_sync", [(4, None), (4, 200), (10, None)])
@pytest.mark.parametrize("kind", ["same", "disjoint"])
@pytest.mark.parametrize("name", skew.SKEWED)
def test_skewed_keys(engine, name, kind, levels, max_sync, mode):
    """Key sets whose buckets hold thousands of rows next to empty ones, and whose bucket
    boundaries the interpolation search does not bracket (tests/skew.py).  The home path
    takes exactly the hops within its limits (run_protocol asserts that from the oracle's
    continuations), and at least one in every case."""
    ra, rb = skew.skewed_pair(name) if kind == "same" else skew.disjoint_pair(name)
    a, b = ra["rows"], rb["rows"]
    sa, sb = side(engine, a, 10), side(engine, b, 10)
    out = P.run_protocol(sa, sb, levels, max_sync, mode, engine)
    check_keys(out, R.store_diff(a, b), sa[1], max_sync)
    if mode == "home":
        assert out["homed"] >= 1
        assert out["homed"] == sum(not P.over_home_limits(rc) for rc in out["conts"])


@pytest.mark.parametrize("mode", MODES)
def test_hot_key(engine, mode):
    """A 20,000-row key in a 20,006-row bucket (far past the 16 rows kept in registers),
    one of its rows with another ts on the other replica: exactly that key."""
    rep, hot = skew.hot_state()
    a = rep["rows"]
    if "hot_b" not in _CACHE:
        i = int(np.searchsorted(a[0], hot)) + 12345
        assert a[0][i] == hot
        ts = a[2].copy()
        ts[i] += 1
        _CACHE["hot_b"] = R.as_rows((a[0], a[1], ts, a[3], a[4]))
        assert R.store_check(_CACHE["hot_b"])  # (values are unique per row: the order stands)
    b = _CACHE["hot_b"]
    sa, sb = side(engine, a, 10), side(engine, b, 10)
    assert sa[1].counts.max() == 20006
    for first, second in ((sa, sb), (sb, sa)):
        out = P.run_protocol(first, second, 4, None, mode, engine)
        assert out["keys"].tolist() == [int(hot)]
        if mode == "home":
            assert out["homed"] == out["hops"]


# ---------------------------------------------------------------- term-hash trees
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as G  # noqa: E402


def _shuffled_universe(state, seed):
    """A Universe that interned the state's values and nodes in a shuffled order first (as
    in test_gpu_term_trees.py)."""
    from oracle.erlterm import tg, untg
    U = Universe()
    vals, nodes = set(), set()
    for entries in state.value.values():
        for (v, _ts), dots in entries.items():
            vals.add(v)
            nodes.update(n for n, _ in dots)
    vals = [untg(x) for x in {tg(v) for v in vals}]
    nodes = sorted(nodes, key=repr)
    rng = random.Random(seed)
    rng.shuffle(vals)
    rng.shuffle(nodes)
    for v in vals:
        U.value(v)
    for n in nodes:
        U.node(n)
    return U


@pytest.fixture(scope="module")
def term_replicas(engine):
    from delta_crdt_ex_amd import aw_lww_map as M
    M._ENGINE = engine
    reps = G.history(210, Universe(), values=G.TERM_VALUES)
    A, B = reps[0], reps[1]
    U1, U2 = _shuffled_universe(A, 1), _shuffled_universe(B, 2)
    sa, sb = M.from_terms(A.value, A.dots, U1), M.from_terms(B.value, B.dots, U2)
    want = sorted(U1.key(k) for k in set(A.value) | set(B.value) if A.value.get(k) != B.value.get(k))
    return M, (sa, U1), (sb, U2), np.array(want, np.uint64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [3, 8])
def test_term_hash_trees(engine, term_replicas, depth, mode):
    """Rows hashed through their terms (dg_term_hashes), each replica with its own interning
    tables: the hops equal the oracle's over each side's own tables, and the keys are those
    whose raw value maps differ."""
    M, (sa, U1), (sb, U2), want = term_replicas
    assert len(want) > 0
    sides = []
    for st, U in ((sa, U1), (sb, U2)):
        rows = st.rows.to_numpy()
        t = M.merkle_map(st, depth)
        r = R.merkle_build(rows, depth, terms=R.Terms(*U.term_tables()))
        assert np.array_equal(u64(t.nodes), r.nodes) and np.array_equal(t.bucket_counts(), r.counts)
        sides.append((t, r, rows))
    for first, second in (sides, sides[::-1]):
        out = P.run_protocol(first, second, 3, None, mode, engine)
        assert np.array_equal(out["keys"], want)
        if mode == "home":
            assert out["homed"] == out["hops"]
