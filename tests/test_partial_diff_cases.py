"""The inputs of tests/test_gpu_partial_diff.py do what that file relies on (CPU, the C
oracle only): the ladder holds every bucket class it names, the oracle's protocol on it
ends in the exact row-set diff, its continuations stay inside the home path's limits (so
"never declined" is a fair assertion there), and the wide pair goes over them."""
import numpy as np
import pytest

import partial_diff_cases as P
from oracle import ref as R

SHARDS = [(0, 0), (2, 1), (2, 3)]
DEPTH = 8


@pytest.mark.parametrize("shard_bits,shard", SHARDS)
def test_ladder_holds_every_class(shard_bits, shard):
    a, b, classes = P.ladder(DEPTH, shard_bits, shard)
    t = R.Tree(DEPTH, shard_bits, shard)
    shift = 64 - shard_bits - DEPTH
    base = (shard << (64 - shard_bits)) if shard_bits else 0
    assert len(classes) == P.N_CLASSES + 2 == 200
    assert {c for c in classes if c[0] != "spare"} == {(s, p, e) for s in P.SIZES for p in range(3)
                                                       for e in range(6)}
    assert len(set(classes.values())) == 200
    for rows in (a, b):  # sorted stores of unique rows inside the shard
        assert R.store_check(rows)
        assert np.all((rows[0] >> np.uint64(64 - shard_bits) if shard_bits else rows[0] * 0) == shard)
        assert rows[1].min() >= 1 << 62 and set(rows[3].tolist()) == {0, 1, 2, 3}
        assert rows[2].min() < 0 < rows[2].max() and len(np.unique(rows[4])) == len(rows[4])
    ba, bb = t.bucket_of(a[0]), t.bucket_of(b[0])
    for cls, bk in classes.items():
        if cls[0] == "spare":
            continue
        size, pattern, edit = cls
        first = base + (bk << shift)
        ka, kb = a[0][ba == bk], b[0][bb == bk]
        assert len(ka) == size
        ua = np.unique(ka)
        assert len(ua) == (size if pattern == 0 else min(size, 1) if pattern == 1 else -(-size // 3))
        if size:
            assert ua[0] == first + 16 and np.all(np.diff(ua) == 16)
        only_a, only_b = np.setdiff1d(ka, kb), np.setdiff1d(kb, ka)
        ra = tuple(c[ba == bk] for c in a)
        rb = tuple(c[bb == bk] for c in b)
        same = all(np.array_equal(x, y) for x, y in zip(ra, rb))
        if edit == 0 or (edit in (1, 2, 5) and size == 0):
            assert same
        elif edit == 1:
            assert not same and len(only_a) == len(only_b) == 0
            assert np.array_equal(R.store_diff(ra, rb), ka[-1:])  # one leaf: the last row's key
        elif edit == 2:
            assert only_a.tolist() == [first + 16] and len(only_b) == 0
            assert (len(kb) == 0) == (len(ua) == 1)  # (pattern 1: B's bucket becomes empty)
            assert pattern != 1 or len(kb) == 0
        elif edit == 3:
            assert only_b.tolist() == [first + 1] and len(only_a) == 0
        elif edit == 4:
            assert only_b.tolist() == [first + (1 << shift) - 1] and len(only_a) == 0
        else:
            assert len(kb) == 0
    first_key, last_key = base, base + (1 << (64 - shard_bits)) - 1
    assert classes[("spare", "first")] == 0 and classes[("spare", "last")] == 255
    assert a[0][0] == first_key and b[0][0] != first_key
    assert b[0][-1] == last_key and a[0][-1] != last_key
    if shard_bits == 0:
        assert first_key == 0 and last_key == (1 << 64) - 1
    # the row counts the kernel's register path steps across
    assert set(R.merkle_build(a, DEPTH, shard_bits, shard).counts.tolist()) == set(P.SIZES) | {3}


@pytest.mark.parametrize("shard_bits,shard", SHARDS)
def test_oracle_protocol_on_the_ladder(shard_bits, shard):
    """The oracle alone: every run ends in store_diff (or, truncated, in the differing keys
    of the buckets kept), and no continuation is over the home path's limits."""
    a, b, _ = P.ladder(DEPTH, shard_bits, shard)
    ra, rb = R.merkle_build(a, DEPTH, shard_bits, shard), R.merkle_build(b, DEPTH, shard_bits, shard)
    full = R.store_diff(a, b)
    assert len(full) > 300
    sides = ((None, ra, a), (None, rb, b))
    biggest = (0, 0)
    for levels in (8, 3, 1):
        for first, second in (sides, sides[::-1]):
            out = P.run_protocol(first, second, levels, None)
            assert np.array_equal(out["keys"], full)
            assert out["hops"] == -(-DEPTH // levels) + 1
            for rc in out["conts"]:
                assert not P.over_home_limits(rc)
            biggest = max([biggest] + out["sizes"])
            for max_sync in (5, 1):
                out = P.run_protocol(first, second, levels, max_sync)
                assert np.all(np.isin(out["keys"], full))  # (possibly none: {:ok, []})
                assert np.array_equal(out["keys"], P.kept_keys(full, ra, out["kept"]))
                assert all(n <= max_sync for n, nb in out["sizes"] if nb == 0)
                assert all(nb <= max_sync for n, nb in out["sizes"])
    assert biggest[0] <= P.HOME_ENTRIES and biggest[1] <= P.HOME_BUCKETS
    assert biggest[1] > 100  # (and far from trivial: most edited buckets in one leaf form)


def test_wide_pair_goes_over_the_home_limits():
    a, b = P.wide_pair()
    assert len(np.unique(a[0])) < len(a[0])  # multi-row keys
    assert len(np.setdiff1d(a[0], b[0])) and len(np.setdiff1d(b[0], a[0]))  # different key sets
    for depth, differing in ((11, 1448), (12, 1900)):
        ra, rb = R.merkle_build(a, depth), R.merkle_build(b, depth)
        assert int((ra.level(depth) != rb.level(depth)).sum()) == differing > P.HOME_BUCKETS
        out = P.run_protocol((None, ra, a), (None, rb, b), depth, None)
        assert np.array_equal(out["keys"], R.store_diff(a, b))
        assert len(out["conts"][0][2]) == 1 << depth <= P.HOME_ENTRIES  # the bucket level fits
        assert out["sizes"][0][1] == differing
        assert P.over_home_limits(out["conts"][1])  # the leaf form does not
