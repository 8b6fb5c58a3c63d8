"""Every entry point that searches a store by key, on key ids that are NOT uniform hashes:
geometric keys, two clusters at the ends of the key space, dense small integers plus one
maximal key, and hashed keys with one key holding a run of 20,000 rows -- with uniform
keys as the control.  The C-ABI takes raw u64 ids and the searches' comments promise
"exact for any key distribution": these inputs send interp_lower_bound to its binary
finish and mp_split to mp_search (tests/test_skew_models.py asserts that they do, on the
same replicas), wave_lower_bound / key_split and wave_find to rounds a hash never needs.
Bit-exact against the C oracle everywhere."""
import numpy as np
import pytest

import skew
from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.store import Store, u64
from lww_diffs_cases import expected_diffs
from oracle import ref as R
from test_gpu_join_delta import apply, kdev
from test_gpu_mutate import run as mutate_run
from test_gpu_parity import DEV, check_join, ctx_eq, rows_eq, up

pytestmark = pytest.mark.gpu

NAMES = list(skew.GENERATORS)
TOP = skew.TOP


def _absent(present, rng, n=40):
    """Keys no row holds: next to present keys, anywhere in the key space, and both ends."""
    near = present[rng.integers(0, len(present), n)]
    near = near[near != np.uint64(TOP)] + np.uint64(1)
    far = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    cand = np.concatenate([near, far, np.array([0, 1, TOP - 1, TOP], np.uint64)])
    return np.setdiff1d(cand, present)


def _keysets(a, b, rng):
    keys = skew.union_keys([a, b])
    return [keys[::2], np.union1d(keys[5::40], _absent(keys, rng))]


def check_changes(engine, a, b, keys=None):
    sa, ca = up(a)
    sb, cb = up(b)
    ks = None if keys is None else np.unique(np.asarray(keys, np.uint64))
    out, octx, ch = engine.join2_changes(sa, ca, sb, cb, keys=None if ks is None else kdev(ks))
    wr, wc = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"], keys=ks)
    rows_eq(out, wr)
    ctx_eq(octx, wc)
    assert np.array_equal(u64(ch), R.changed_keys(a["rows"], wr, ks))


# ---------------------------------------------------------------- join2 / join2_changes

@pytest.mark.parametrize("name", NAMES)
def test_join2_same_key_set(engine, name):
    """Both replicas on one skewed key set, both orders: unkeyed, every second key, and a
    sparse keyset with absent keys (key_split's wave_lower_bound over a skewed keyset)."""
    a, b = skew.skewed_pair(name)
    rng = np.random.default_rng(1)
    for x, y in ((a, b), (b, a)):
        check_join(engine, x, y)
        check_changes(engine, x, y)
        for ks in _keysets(a, b, rng):
            check_join(engine, x, y, keys=ks)
            check_changes(engine, x, y, keys=ks)


@pytest.mark.parametrize("name,n_keys", [(n, skew.BASE_KEYS) for n in NAMES] + [("geometric", skew.BIG_KEYS)])
def test_join2_different_key_sets(engine, name, n_keys):
    """A on the skewed key set, B an independent replica on uniform keys, none shared: the
    merge-path split is nowhere near the gap-shifted guess, so the tile boundaries go
    through mp_search (both orders, and keyed)."""
    a, b = skew.disjoint_pair(name, n_keys)
    rng = np.random.default_rng(2)
    for x, y in ((a, b), (b, a)):
        check_join(engine, x, y)
        for ks in _keysets(a, b, rng):
            check_join(engine, x, y, keys=ks)
    check_changes(engine, a, b)
    check_changes(engine, b, a, keys=_keysets(a, b, rng)[1])


@pytest.mark.parametrize("name", NAMES)
def test_sparse_keyed_join_takes_the_splice(engine, name):
    """(|K| + |B|) * 8 <= |A| with A at 20,000 keys: the splice locates K's keys in A
    (its index: interp_lower_bound per key) instead of merging the whole state."""
    a, b = skew.skewed_pair(name, skew.BIG_KEYS)
    rng = np.random.default_rng(3)
    keys = skew.union_keys([a, b])
    ks = np.union1d(rng.choice(keys, 800, replace=False), _absent(keys, rng))
    d = W.sync_delta(b, ks)
    assert 0 < (len(ks) + len(d["rows"][0])) * 8 <= len(a["rows"][0])
    check_changes(engine, a, d, keys=ks)
    check_join(engine, a, d, keys=ks)


# ---------------------------------------------------------------- take_keys, reads

def _states(name):
    return skew.hot_state()[0] if name == "hot_key" else skew.skewed_pair(name)[0]


@pytest.mark.parametrize("name", NAMES + ["hot_key"])
def test_take_keys(engine, name):
    """Map.take of every key, every 7th, key + 1 (absent) and the first and last five,
    against the host's np.isin (W.sync_delta)."""
    a = _states(name)
    s, _ = up(a)
    for what, ks in skew.take_lists(a["rows"][0]).items():
        got = engine.take_keys(s, kdev(ks))
        want = W.sync_delta(a, ks)["rows"]
        assert got.n == len(want[0]), (what, got.n, len(want[0]))
        rows_eq(got, want)


@pytest.mark.parametrize("name", NAMES + ["hot_key"])
def test_read_diff_and_keyed_read(engine, name):
    """read/2 of key lists before and after a join (dg_read_diff) and dg_read_lww with keys:
    every key, absent keys (0 with the flag clear), in any order for read_diff."""
    rng = np.random.default_rng(4)
    if name == "hot_key":
        a = skew.hot_state()[0]
        new = tuple(c[::2] for c in a["rows"])  # (still sorted and unique; the hot key keeps 10,000 rows)
    else:
        a, b = skew.skewed_pair(name)
        new, _ = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"])
    old = a["rows"]
    present = np.unique(np.concatenate([old[0], new[0]]))
    absent = _absent(present, rng)
    so, sn = Store.from_numpy(*old, device=DEV), Store.from_numpy(*new, device=DEV)
    for ks in (present, absent, rng.permutation(np.concatenate([present[::3], absent, present[:30]]))):
        got = engine.read_diff(so, sn, kdev(ks))
        want = expected_diffs(old, new, ks)
        for nm, x, y in zip(("old_val", "new_val", "flags"), got, want):
            assert np.array_equal(x.cpu().numpy().view(y.dtype), y), nm
    gv, gn, gf = engine.read_diff(so, sn, kdev(absent))
    assert not gv.any() and not gn.any() and not gf.any()
    for rows, st in ((old, so), (new, sn)):
        for ks in (present, np.union1d(present[::5], absent), absent):
            ok, ov = engine.read_lww(st, keys=kdev(ks))
            wk, wv = R.read_lww(rows, keys=ks)
            assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)
    assert engine.read_lww(so, keys=kdev(absent))[0].numel() == 0


# ---------------------------------------------------------------- join_delta

@pytest.mark.parametrize("home", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_join_delta_300_keys(engine, name, home):
    """A 300-key sync delta into a resident state with a depth-10 tree: the small path
    (home) and dg_join_delta_rows; state, context, changed keys, their rows, and the tree,
    its bucket counts and chunk index equal to a fresh build (apply asserts them)."""
    a, b = skew.skewed_pair(name)
    rng = np.random.default_rng(5)
    # 300 keys in a random order of the union, passing over a key whose rows would take the
    # delta past the 512 rows the small path accepts (B holds about two rows per key, so the
    # last sixty or so are keys B has no row for: removals only)
    ub, cb = np.unique(b["rows"][0], return_counts=True)
    rows_of = dict(zip(ub.tolist(), cb.tolist()))
    keys, n_rows = [], 0
    for k in rng.permutation(skew.union_keys([a, b])).tolist():
        if n_rows + rows_of.get(k, 0) <= 512:
            keys.append(k)
            n_rows += rows_of.get(k, 0)
            if len(keys) == 300:
                break
    keys = np.sort(np.array(keys, np.uint64))
    d = W.sync_delta(b, keys)
    assert len(keys) == 300 and 400 < len(d["rows"][0]) <= 512
    apply(engine, a, d, keys, depth=10, home=home)


@pytest.mark.parametrize("name", NAMES)
def test_join_delta_3000_keys(engine, name):
    """3,000 keys: the one-wait per-key path (kd_count_kernel's lookups, the Merkle update)."""
    a, b = skew.skewed_pair(name)
    rng = np.random.default_rng(6)
    keys = np.sort(rng.choice(skew.union_keys([a, b]), 3000, replace=False))
    apply(engine, a, W.sync_delta(b, keys), keys, depth=10)


@pytest.mark.parametrize("others,depth", [("far", 10), ("same bucket", 6)])
def test_join_delta_names_the_hot_key(engine, others, depth):
    """A delta that names the key with 20,000 rows (over KD_RUN: the per-key path hands
    over, and undoes what it put into the tree) and a key on either side of it -- far away,
    or its neighbours in its own bucket; its VV covers half of every node's dots, so half
    of the hot key's rows go and the delta's row joins them.
    (The `far` case found kd_count_kernel's tree_put adding the first key's row-count
    change to the chunk index twice, the undo taking it out once: starts[1] one too many.)"""
    a, hot = skew.hot_state()
    keys = np.unique(a["rows"][0])
    i = int(np.searchsorted(keys, hot))
    if others == "far":
        dk = np.array([keys[5], hot, keys[len(keys) - 7]], np.uint64)
    else:
        dk = np.array([keys[i - 1], hot, keys[i + 1]], np.uint64)
        assert len(set((dk >> np.uint64(64 - depth)).tolist())) == 1
    half = int(a["ctx"][2][0]) // 2
    d = {"rows": (dk, np.array([7, 8, 9], np.uint64), np.full(3, 10 ** 6, np.int64), np.full(3, 7, np.uint32),
                  np.array([1, 2, 3], np.uint64)),
         "ctx": (R.VV, np.array([0, 1, 2, 3, 7], np.uint32), np.array([half, half, half, half, 3], np.uint64))}
    _, _, swapped, wr = apply(engine, a, d, dk, depth=depth)
    assert swapped and 0 < int((wr[0] == hot).sum()) < skew.HOT_RUN


# ---------------------------------------------------------------- mutate_batch

@pytest.mark.parametrize("name", NAMES)
def test_mutate_batch(engine, name):
    """400 ops of one node: adds on existing keys, adds on new keys inside the clusters
    (key + 1) and between them, removes of present and absent keys."""
    a, _ = skew.skewed_pair(name)
    rng = np.random.default_rng(7)
    keys = np.unique(a["rows"][0])
    absent = _absent(keys, rng, n=200)
    ops = []
    for i in range(400):
        r = rng.random()
        k = int(rng.choice(keys)) if r < 0.5 or 0.8 <= r < 0.9 else int(rng.choice(absent))
        if r < 0.8:
            ops.append(("add", k, int(rng.integers(0, 9)) + (1 << 62), 10 ** 12 + i))
        else:
            ops.append(("remove", k, 0, 0))
    drows, dctx, dkeys = mutate_run(engine, a, 2, ops)
    wr, wc, wk = R.mutate_batch(a["rows"], a["ctx"], 2, ops)
    rows_eq(drows, wr)
    ctx_eq(dctx, wc)
    assert np.array_equal(u64(dkeys), wk)
    s, c = up(a)
    out, octx = engine.join2(s, c, drows, dctx, keys=dkeys)
    jr, jc = R.join2(a["rows"], a["ctx"], wr, wc, wk)
    rows_eq(out, jr)
    ctx_eq(octx, jc)


# ---------------------------------------------------------------- Merkle

@pytest.mark.parametrize("name", NAMES + ["hot_key"])
def test_merkle_build_diff_update(engine, name):
    """dg_merkle_build at depth 10 against the oracle's tree (every bucket below 65,536
    rows at these sizes), dg_merkle_diff against the store diff, and dg_merkle_update after
    the join equal to a fresh build."""
    if name == "hot_key":
        a = skew.hot_state()[0]
        b = {"rows": tuple(c[::2] for c in a["rows"]), "ctx": a["ctx"]}
    else:
        a, b = skew.skewed_pair(name)
    sa, ca = up(a)
    sb, cb = up(b)
    ta, tb = engine.merkle_build(sa, 10), engine.merkle_build(sb, 10)
    for t, rep in ((ta, a), (tb, b)):
        r = R.merkle_build(rep["rows"], 10)
        assert t.n_keys == r.n_keys
        assert np.array_equal(t.nodes.cpu().numpy().view(np.uint64), r.nodes)
        assert np.array_equal(t.bucket_counts(), r.counts)
    want = R.store_diff(a["rows"], b["rows"])
    assert len(want) > 0
    assert np.array_equal(u64(engine.merkle_diff(ta, tb)), want)
    assert np.array_equal(u64(engine.merkle_diff(tb, ta)), want)
    out, octx, changed = engine.join2_changes(sa, ca, sb, cb)
    engine.merkle_update(ta, out, changed)
    fresh = engine.merkle_build(out, 10)
    assert np.array_equal(ta.nodes.cpu().numpy(), fresh.nodes.cpu().numpy())
    assert np.array_equal(ta.bucket_counts(), fresh.bucket_counts())
    assert ta.n_keys == fresh.n_keys
