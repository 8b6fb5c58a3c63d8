"""The CPU models of interp_lower_bound and mp_split (tests/skew.py) are exact, and the
inputs tests/test_gpu_skewed_keys.py runs on the device do leave the paths tuned for hashed
keys: without these reach conditions the GPU tests could pass without ever executing the
fallbacks they are there for."""
import numpy as np
import pytest

import skew
from skew import TOP


def _queries(keys, rng, n=400):
    sel = keys if len(keys) <= 2000 else np.sort(rng.choice(keys, n, replace=False))
    nxt = sel[sel != np.uint64(TOP)] + np.uint64(1)  # absent, or the next key of a dense set
    return np.concatenate([sel, nxt, np.array([0, TOP], np.uint64)])


@pytest.mark.parametrize("n", [2_000, 20_000])
@pytest.mark.parametrize("name", list(skew.GENERATORS))
def test_generators_and_interp_model(name, n):
    rng = np.random.default_rng(n)
    keys = skew.GENERATORS[name](rng, n)
    assert keys.dtype == np.uint64 and len(keys) == n and bool(np.all(keys[1:] > keys[:-1]))
    if name == "two_clusters":
        assert keys[0] == 0 and keys[-1] == TOP
        assert int((keys < (1 << 24)).sum()) == n // 2 and int((keys >= np.uint64(TOP - (1 << 24) + 1)).sum()) == n - n // 2
    q = _queries(keys, rng)
    kl = keys.tolist()
    got = np.array([skew.model_interp_lower_bound(kl, int(x))[0] for x in q])
    assert np.array_equal(got, np.searchsorted(keys, q, side="left"))
    # and over a key column with runs (several rows per key), as the stores have
    col = np.repeat(keys, rng.integers(1, 4, n))
    cl = col.tolist()
    got = np.array([skew.model_interp_lower_bound(cl, int(x))[0] for x in q])
    assert np.array_equal(got, np.searchsorted(col, q, side="left"))


def test_interp_model_edges():
    assert skew.model_interp_lower_bound([], 5) == (0, "early")
    assert skew.model_interp_lower_bound([7], 7) == (0, "early")
    assert skew.model_interp_lower_bound([7], 8) == (1, "early")
    k = list(range(0, 170, 10))  # 17 keys: b - a = 16, the window at once
    for x in range(0, 175):
        i, path = skew.model_interp_lower_bound(k, x)
        assert i == int(np.searchsorted(np.array(k), x)) and path in ("early", "window")


@pytest.mark.parametrize("n", [2_000, 20_000])
@pytest.mark.parametrize("name", list(skew.GENERATORS))
def test_mp_split_model(name, n):
    rng = np.random.default_rng(n + 1)
    a = skew.GENERATORS[name](rng, n)
    b = skew.uniform(rng, n + 64)
    b = b[~np.isin(b, a)][:n]
    # key columns with runs, as the stores have
    A, B = np.repeat(a, rng.integers(1, 4, n)), np.repeat(b, rng.integers(1, 3, n))
    total = len(A) + len(B)
    ds = sorted(set(skew.boundaries(len(A), len(B))) | set(range(0, total + 1, max(1, total // 60))) | {1, total - 1, total})
    for X, Y in ((A, B), (B, A)):
        xl, yl = X.tolist(), Y.tolist()
        from_x = np.argsort(np.concatenate([X, Y]), kind="stable") < len(X)
        cum = np.concatenate([[0], np.cumsum(from_x)])
        paths = set()
        for d in ds:
            s, path = skew.model_mp_split(xl, yl, d)
            assert s == int(cum[d]), (name, n, d, path)
            paths.add(path)
        assert paths <= {"short", "win0", "win1", "win2", "search"}
    assert skew.true_split(B, A, ds[3]) == int(cum[ds[3]])


def test_true_split_small():
    A, B = np.array([1, 1, 5, 9], np.uint64), np.array([2, 3, 3, 10], np.uint64)
    assert [skew.true_split(A, B, d) for d in range(9)] == [0, 1, 2, 2, 2, 2, 3, 4, 4]
    for d in range(9):
        assert skew.model_mp_split(A, B, d) == (skew.true_split(A, B, d), "short")


# ---------------------------------------------------------------- reach conditions
# On exactly the inputs of tests/test_gpu_skewed_keys.py (same generator, size and seed,
# built by the same skew.py functions).

def _frac(paths, which):
    return sum(p == which for p in paths) / max(len(paths), 1)


@pytest.mark.parametrize("name", list(skew.GENERATORS))
def test_base_replicas_reach_the_binary_finish(name):
    a, b = skew.skewed_pair(name)
    for rep in (a, b):
        col = rep["rows"][0]
        paths = skew.interp_paths(col, skew.take_lists(col)["every 7th"])
        print(name, len(col), "rows:", {p: paths.count(p) for p in set(paths)})
        if name == "uniform":
            assert "binary" not in paths
            for ks in skew.take_lists(col).values():
                assert "binary" not in skew.interp_paths(col, ks)
        else:
            assert _frac(paths, "binary") >= 0.5


def test_hot_key_reaches_the_binary_finish():
    st, hot = skew.hot_state()
    col = st["rows"][0]
    others = np.unique(col)
    others = others[others != hot][::7]
    paths = skew.interp_paths(col, others)
    print("hot key:", {p: paths.count(p) for p in set(paths)})
    assert _frac(paths, "binary") >= 0.2
    assert int((col == hot).sum()) == skew.HOT_RUN


@pytest.mark.parametrize("name,n_keys,floor", [("uniform", skew.BASE_KEYS, None),
                                                ("uniform", skew.BIG_KEYS, None),
                                                ("two_clusters", skew.BASE_KEYS, 0.5),
                                                ("geometric", skew.BIG_KEYS, 0.5)])
def test_disjoint_replicas_reach_mp_search(name, n_keys, floor):
    a, b = skew.disjoint_pair(name, n_keys)
    A, B = a["rows"][0], b["rows"][0]
    assert not np.isin(A, B).any()
    for X, Y in ((A, B), (B, A)):
        paths = skew.split_paths(X, Y)
        print(name, n_keys, {p: paths.count(p) for p in set(paths)})
        assert len(paths) >= 9
        if floor is None:
            assert "search" not in paths
        else:
            assert _frac(paths, "search") >= floor
