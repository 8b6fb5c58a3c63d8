"""The inputs of tests/test_gpu_take_passes.py do what that file relies on (CPU, the C oracle and
numpy only): the hops of take_pass_cases.CASES -- the very list the GPU cases run -- reach every
situation of the take hop's pass loop between them, none of them is over the home path's limits,
and huge()'s three cuts give the row totals around 2^22.

huge() takes 1.1 s of numpy to build here (4,194,305 rows, one lexsort), its three expectations
0.04 s each."""
import numpy as np

import cont_batch_cases as B
import partial_diff_cases as P
import take_pass_cases as T
from oracle import ref as R


def test_stairs_layout():
    rows_x, rows_p = T.stairs()
    assert R.store_check(rows_x) and R.store_check(rows_p)
    assert len(rows_x[0]) == T.X_ROWS and 4 * T.PASS < T.X_ROWS <= 4 * T.ROOM_KEYS + T.ROOM_EXTRA
    assert len(np.unique(rows_p[0])) <= P.HOME_ENTRIES
    counts = B.tree_of(rows_x, T.DEPTH).counts.astype(np.int64)
    assert counts[T.LONG_BUCKET] == T.LONG_ROWS > 2 * T.PASS
    assert len(np.unique(rows_x[0][rows_x[0] >> np.uint64(T.SHIFT) == T.LONG_BUCKET])) == 1
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]  # a bucket's first row
    reg, big = (counts > 0) & (counts <= T.BR), (counts > T.BR) & (counts <= 40)
    assert reg.sum() + big.sum() == T.NBK - 1
    for bnd in (T.PASS, 2 * T.PASS, 3 * T.PASS):  # both kinds on both sides of every boundary
        for kind in (reg, big):
            assert np.any(kind & (first + counts <= bnd)) and np.any(kind & (first >= bnd))
    assert first[T.LONG_BUCKET] > T.PASS  # a cut before the long key can keep more than one pass
    per_key = np.unique(rows_x[0], return_counts=True)[1]
    small = per_key[per_key != T.LONG_ROWS]
    assert {1, 3, 5} <= set(small.tolist()) and small.max() == 5
    # P's edits: identical keys, keys only one side holds, an empty bucket, one row's ts
    px, pp = np.unique(rows_x[0]), np.unique(rows_p[0])
    diff = R.store_diff(rows_x, rows_p)
    assert len(np.setdiff1d(px, pp)) and len(np.setdiff1d(pp, px)) and len(np.setdiff1d(px, diff))
    assert not np.any(diff >> np.uint64(T.SHIFT) < 8)  # the first buckets identical
    assert np.any(np.bincount((rows_p[0] >> np.uint64(T.SHIFT)).astype(np.int64), minlength=T.NBK)[counts > 0] == 0)
    long_rows = np.flatnonzero(rows_x[0] >> np.uint64(T.SHIFT) == T.LONG_BUCKET)
    by_cnt = np.argsort(rows_p[4])  # (cnt is unique: P's row of the same dot)
    theirs = by_cnt[np.searchsorted(rows_p[4][by_cnt], rows_x[4][long_rows])]
    bump = rows_p[2][theirs] - rows_x[2][long_rows]
    assert not bump[:-1].any() and bump[-1] == 1  # the long key: its last row's ts alone


def test_cases_reach_every_pass_situation():
    rows_x, _ = T.stairs()
    reached = set()
    for max_sync in T.CASES:
        hops = T.hops(max_sync)
        assert not any(P.over_home_limits(rc) for rc, _ in hops)
        kinds = [B.kind_of(w) for _, w in hops]
        assert {"node", "leaf", "keys"} <= set(kinds)
        assert kinds[-len(T.CRAFTED):] == ["keys"] * len(T.CRAFTED)
        reached |= T.pass_paths(rows_x, hops, max_sync)
    assert reached == T.SITUATIONS
    # the totals the GPU cases pick hops by
    totals = [T.row_total(rows_x, w[1]) for _, w in T.hops(None) if B.kind_of(w) == "keys"]
    assert {T.PASS, T.PASS + 1, 2 * T.PASS, T.X_ROWS} <= set(totals)
    assert any(3 * T.PASS < t <= 4 * T.PASS for t in totals)  # four passes


def test_replica_room_serves_the_largest_hop():
    """replica_pack.h rp_take_room_for: min(rows_n, 4 * min(kcap, 4096) + 64) rows, kcap =
    min(max_sync, rows_n + n + 1, 65536) keys (rp_cont_room_for).  Unbounded, the largest keys hop
    of the conversations -- all of X, the long key with it -- has room.  At the cut the long key
    alone is over four rows a key: the hop against P, which holds it, is over the room and takes
    the fallback, and the hop against the empty replica, cut before the long key, is the
    multi-pass hop the launch serves."""
    rows_x, _ = T.stairs()
    long_key = np.uint64((T.LONG_BUCKET << T.SHIFT) + T.STEP)
    for max_sync in T.CASES:
        hops = [(T.row_total(rows_x, T.kept_of(w, max_sync)), len(rc[2]), long_key in T.kept_of(w, max_sync))
                for rc, w in T.hops_of_conversations(max_sync) if B.kind_of(w) == "keys"]
        fits = [need <= T.replica_room(len(rows_x[0]), n_in, max_sync) for need, n_in, _ in hops]
        if max_sync is None:
            assert max(hops)[0] == T.X_ROWS and fits[hops.index(max(hops))] and max(hops)[2]
        else:
            assert [h[2] for h in hops] == [not f for f in fits] == [True, False]
            assert hops[1][0] > T.PASS


def test_huge_totals():
    rows = T.huge()
    assert R.store_check(rows) and len(rows[0]) == T.HUGE_ROWS == (1 << 22) + 1
    counts = np.bincount((rows[0] >> np.uint64(T.SHIFT)).astype(np.int64), minlength=T.NBK)
    assert counts.max() <= 65535 and counts.min() == 8192  # a bucket's row count is a u16
    want = {1023: (1 << 22) - 1, 1024: 1 << 22, None: (1 << 22) + 1}
    assert T.HUGE_CUTS == tuple(want)
    for max_sync, total in want.items():
        kept, n_keys, rows_kept = T.huge_expect(rows, max_sync)
        assert n_keys == 1025 and len(kept) == min(1025, max_sync or 1025) and rows_kept == total
        assert rows_kept == int(np.isin(rows[0], kept).sum())
    dots = rows[3].astype(np.uint64) << np.uint64(40) | rows[4]
    assert len(np.unique(dots)) == T.HUGE_ROWS
