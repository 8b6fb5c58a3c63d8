"""dg_store_diff (csrc/sdiff.hip) on cuda:0: the streaming diff of two stores against the C
oracle -- the changed keys against ref_store_diff, the winners on either side against
ref_read_lww (through lww_diffs_cases.expected_diffs), the rows against the rows of the new
store under those keys.  The shapes are the ones at which the kernels take another path:
empty sides, a key differing in exactly one way, a run starting just before a tile's
diagonal, runs longer than a tile (the workgroup-wide compare, empty tiles), tile counts
around the scan's 1024 stretches, keys that are not hashes."""
import numpy as np
import pytest
import torch

import skew
from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd._abi import CapacityError
from delta_crdt_ex_amd.interning import splitmix64_np
from delta_crdt_ex_amd.store import Store, u64
from lww_diffs_cases import expected_diffs
from oracle import ref as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

TOP = np.uint64((1 << 64) - 1)


def rows_of(tuples):
    """Sorted unique SoA rows from (key, val, ts, node, cnt) tuples."""
    if not tuples:
        return R.empty_rows()
    t = sorted(set(tuples))
    return (np.array([x[0] for x in t], np.uint64), np.array([x[1] for x in t], np.uint64),
            np.array([x[2] for x in t], np.int64), np.array([x[3] for x in t], np.uint32),
            np.array([x[4] for x in t], np.uint64))


def cat(*parts):
    """Row sets over disjoint key ranges, given in ascending order."""
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))


def singles(keys, salt=0):
    """One row per key."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    i = np.arange(n, dtype=np.uint64)
    return (keys, i % np.uint64(7) + np.uint64(salt), (i % np.uint64(5)).astype(np.int64),
            (i % np.uint64(3)).astype(np.uint32), i + np.uint64(1))


def run_rows(key, n, last_cnt=None):
    """n rows of one key (distinct vals: the order is the val order); last_cnt: the last
    row's counter (rows that differ in their last row only)."""
    i = np.arange(n, dtype=np.uint64)
    cnt = i + np.uint64(1)
    if last_cnt is not None:
        cnt[-1] = last_cnt
    return (np.full(n, key, np.uint64), i + np.uint64(10), (i % np.uint64(4)).astype(np.int64),
            np.zeros(n, np.uint32), cnt)


def check(engine, a, b):
    """Every output of dg_store_diff(a, b) against the oracle; returns the changed keys."""
    sa, sb = Store.from_numpy(*a, device=DEV), Store.from_numpy(*b, device=DEV)
    changed, rows, (ov, nv, fl) = engine.store_diff(sa, sb, want_rows=True, want_diffs=True)
    want = R.store_diff(a, b)
    assert np.array_equal(u64(changed), want)
    wo, wn, wf = expected_diffs(a, b, want)
    assert np.array_equal(u64(ov), wo), "old_val"
    assert np.array_equal(u64(nv), wn), "new_val"
    assert np.array_equal(fl.cpu().numpy(), wf), "flags"
    m = np.isin(b[0], want)
    assert rows.n == int(m.sum())
    for i, (x, y) in enumerate(zip(rows.to_numpy(), b)):
        assert np.array_equal(x, y[m]), f"rows column {i}"
    # the plain call (no rows, no diffs) gives the same keys
    assert torch.equal(engine.store_diff(sa, sb), changed)
    return want


def test_empty_identical_disjoint(engine):
    e = R.empty_rows()
    ks = np.unique(splitmix64_np(np.arange(1, 3001, dtype=np.uint64)))
    a = singles(ks)
    assert len(check(engine, e, e)) == 0
    assert len(check(engine, a, e)) == len(ks)
    assert len(check(engine, e, a)) == len(ks)
    assert len(check(engine, a, a)) == 0
    assert len(check(engine, singles(ks[::2]), singles(ks[1::2]))) == len(ks)
    # b = a less its last key, plus a key before the first and one after the last
    b = cat(singles([ks[0] - np.uint64(1)]), tuple(c[:-1] for c in a), singles([ks[-1] + np.uint64(1)]))
    assert len(check(engine, a, b)) == 3


def test_keys_zero_and_max(engine):
    mid = np.unique(splitmix64_np(np.arange(1, 2500, dtype=np.uint64)))
    mid = mid[(mid != 0) & (mid != TOP)]
    a = cat(singles([0]), singles(mid), singles([TOP]))
    b = cat(singles([0], salt=1), singles(mid), singles([TOP], salt=1))
    assert np.array_equal(check(engine, a, b), np.array([0, TOP], np.uint64))
    assert np.array_equal(check(engine, a, cat(singles(mid))), np.array([0, TOP], np.uint64))
    assert np.array_equal(check(engine, cat(singles(mid)), a), np.array([0, TOP], np.uint64))
    assert len(check(engine, a, a)) == 0
    # runs of both, longer than one row
    a2 = cat(run_rows(0, 5), singles(mid), run_rows(TOP, 70))
    b2 = cat(run_rows(0, 5, last_cnt=99), singles(mid), run_rows(TOP, 70, last_cnt=99))
    assert np.array_equal(check(engine, a2, b2), np.array([0, TOP], np.uint64))


ONE_KEY = {
    "val": ([(50, 7, 3, 1, 4)], [(50, 8, 3, 1, 4)]),
    "ts": ([(50, 7, 3, 1, 4)], [(50, 7, 4, 1, 4)]),
    "node": ([(50, 7, 3, 1, 4)], [(50, 7, 3, 2, 4)]),
    "cnt": ([(50, 7, 3, 1, 4)], [(50, 7, 3, 1, 5)]),
    "row added": ([(50, 7, 3, 1, 4)], [(50, 7, 3, 1, 4), (50, 9, 2, 1, 5)]),
    "row removed": ([(50, 7, 3, 1, 4), (50, 9, 2, 1, 5)], [(50, 9, 2, 1, 5)]),
    # equal ts: the smallest value id is read (the first row)
    "tie": ([(50, 7, 3, 1, 4)], [(50, 7, 3, 1, 4), (50, 5, 3, 2, 1), (50, 6, 3, 2, 2)]),
    "tie both sides": ([(50, 7, 3, 1, 4), (50, 8, 3, 1, 5)], [(50, 7, 3, 1, 4), (50, 8, 3, 1, 6)]),
}


@pytest.mark.parametrize("case", sorted(ONE_KEY))
def test_one_key_one_way(engine, case):
    """A key differing in exactly one way, alone and among unchanged neighbours, first,
    in the middle and last."""
    ka, kb = ONE_KEY[case]
    assert np.array_equal(check(engine, rows_of(ka), rows_of(kb)), np.array([50], np.uint64))
    around = [(k, 1, 1, 1, k) for k in (10, 20, 30, 60, 70)]
    assert np.array_equal(check(engine, rows_of(ka + around), rows_of(kb + around)), np.array([50], np.uint64))
    lo = [(k, 1, 1, 1, k + 100) for k in range(100, 400)]
    for rest in (lo, [(k - 99, *r) for k, *r in lo if k - 99 < 50]):
        assert np.array_equal(check(engine, rows_of(ka + rest), rows_of(kb + rest)), np.array([50], np.uint64))
    if case == "tie":
        _, nv, _ = expected_diffs(rows_of(ka), rows_of(kb), np.array([50], np.uint64))
        assert nv[0] == 5


SEAMS = [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]


@pytest.mark.parametrize("p", SEAMS)
def test_tile_seams(engine, p):
    """A key whose run of 2, 64 and 65 rows starts 1 and 64 merged rows before merged row p
    (whatever the tile size is, a power of two between 256 and 4096, some of these runs
    straddle a diagonal): only in a, only in b, and in both with a different last row.
    The rows before and after the run are the same in both stores."""
    for off in (1, 64):
        start = p - off  # merged rows before the run: pairs of equal rows, and one row of a alone
        pairs, odd = divmod(start, 2)
        base = np.arange(1, pairs + 401, dtype=np.uint64) * np.uint64(1000)
        head, tail = singles(base[:pairs]), singles(base[pairs:], salt=3)
        extra = [singles([5])] if odd else []
        key = base[pairs - 1] + np.uint64(1) if pairs else np.uint64(7)
        for run in (2, 64, 65):
            for mode in ("a", "b", "both"):
                ra = [run_rows(key, run)] if mode != "b" else []
                rb = [run_rows(key, run, last_cnt=10**6 if mode == "both" else None)] if mode != "a" else []
                a = cat(*extra, head, *ra, tail)
                b = cat(head, *rb, tail)
                want = check(engine, a, b)
                assert key in want and len(want) == 1 + odd, (off, run, mode)


def test_long_runs(engine):
    """Runs longer than a tile: 5,000 rows against 3, and 70,000 rows in both that differ in
    one row in the middle; unchanged and changed short keys on either side."""
    ks = np.unique(splitmix64_np(np.arange(1, 6001, dtype=np.uint64)))
    lo, mid, hi = ks[:2000], ks[2000:4000], ks[4000:]
    k1, k2 = lo[-1] + np.uint64(1), mid[-1] + np.uint64(1)
    big = run_rows(k2, 70_000)
    big2 = tuple(c.copy() for c in big)
    big2[4][35_000] = 10**7  # (the counter: the order of the rows stays)
    a = cat(singles(lo), run_rows(k1, 5000), singles(mid), big, singles(hi))
    b = cat(singles(lo), run_rows(k1, 3), singles(mid, salt=1), big2, singles(hi))
    want = check(engine, a, b)
    assert k1 in want and k2 in want and len(want) == 2 + len(mid)
    # the same runs unchanged, and removed / added whole
    assert len(check(engine, a, a)) == 0
    c = cat(singles(lo), singles(mid), singles(hi))
    assert np.array_equal(check(engine, a, c), np.array([k1, k2], np.uint64))
    assert np.array_equal(check(engine, c, a), np.array([k1, k2], np.uint64))


@pytest.mark.parametrize("tiles", [1023, 1024, 1025])
def test_scan_seams(engine, tiles):
    """About 1023, 1024 and 1025 tiles of 2048 merged rows -- one stretch of the scan's 1024
    threads each, and the step to two tiles per stretch -- with 1 % of the keys changed."""
    n = tiles * 1024 - 512
    rng = np.random.default_rng(tiles)
    ks = np.unique(rng.integers(0, 1 << 64, n + n // 50, dtype=np.uint64))[:n]
    assert len(ks) == n
    a = singles(ks)
    b = tuple(c.copy() for c in a)
    hit = rng.random(n) < 0.01
    b[1][hit] += np.uint64(100)
    sa, sb = Store.from_numpy(*a, device=DEV), Store.from_numpy(*b, device=DEV)
    changed, (ov, nv, fl) = engine.store_diff(sa, sb, want_diffs=True)
    assert np.array_equal(u64(changed), R.store_diff(a, b))
    assert np.array_equal(u64(changed), ks[hit])
    assert np.array_equal(u64(ov), a[1][hit]) and np.array_equal(u64(nv), b[1][hit])
    assert bool((fl == 3).all())


@pytest.mark.parametrize("name", skew.SKEWED)
def test_skewed_keys(engine, name):
    """Unhashed and clustered key sets (tests/skew.py), overlapping and disjoint replicas."""
    a, b = skew.skewed_pair(name)
    assert 0 < len(check(engine, a["rows"], b["rows"]))
    a, b = skew.disjoint_pair(name)
    check(engine, a["rows"], b["rows"])
    check(engine, b["rows"], a["rows"])


def test_hot_key(engine):
    """A key holding 20,000 of a state's rows, against the state less every third row of it."""
    st, hot = skew.hot_state()
    a = st["rows"]
    w = np.flatnonzero(a[0] == hot)
    keep = np.ones(len(a[0]), bool)
    keep[w[::3]] = False
    b = tuple(c[keep] for c in a)
    assert np.array_equal(check(engine, a, b), np.array([hot], np.uint64))
    assert np.array_equal(check(engine, b, a), np.array([hot], np.uint64))


def test_capacity(engine):
    rng = np.random.default_rng(9)
    a, b = W.random_pair(rng, 4000, n_nodes=5, ts_range=8)
    a, b = a["rows"], b["rows"]
    total = len(R.store_diff(a, b))
    assert total > 10
    sa, sb = Store.from_numpy(*a, device=DEV), Store.from_numpy(*b, device=DEV)
    with pytest.raises(CapacityError, match=f"{total} changed keys"):
        engine.store_diff(sa, sb, changed=torch.empty(total - 1, dtype=torch.int64, device=DEV))
    exact = engine.store_diff(sa, sb, changed=torch.empty(total, dtype=torch.int64, device=DEV))
    assert np.array_equal(u64(exact), R.store_diff(a, b))
    # too few rows is not an error of the diff: the rows are not written, their number is
    with pytest.raises(CapacityError, match="rows"):
        engine.store_diff(sa, sb, want_rows=True, rows=Store.empty(3, DEV))
