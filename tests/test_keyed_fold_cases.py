"""The crafted batches of tests/keyed_fold_cases.py do what they are named for: the C
oracle's delta-by-delta fold shows the property each case exists to exercise, so that
tests/test_gpu_join_deltas_keyed.py passing on a case means something.  No GPU."""
import numpy as np

import keyed_fold_cases as KC
from oracle import ref as R


def fold(st, ds, upto=None):
    ds = ds if upto is None else ds[:upto]
    return R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds], [d["ctx"] for d in ds],
                          [d["keys"] for d in ds])


def every_row_in_its_keyset(ds):
    return all(np.isin(d["rows"][0], d["keys"]).all() for d in ds)


def counts(rows, keys):
    return np.array([int((rows[0] == k).sum()) for k in keys])


def test_net_no_change():
    st, ds, K, L = KC.net_no_change()
    assert every_row_in_its_keyset(ds)
    mid, _ = fold(st, ds, 1)
    end, _ = fold(st, ds)
    assert K in R.store_diff(st["rows"], mid) and K in R.store_diff(mid, end)
    assert np.array_equal(R.store_diff(st["rows"], end), np.array([L], np.uint64))


def test_order_dependence():
    st, ds, x, r = KC.order_dependence()
    assert every_row_in_its_keyset(ds)
    assert x not in ds[0]["keys"] and r in KC.key_rows(st["rows"], x) and r in KC.key_rows(ds[1]["rows"], x)
    assert r not in KC.key_rows(ds[0]["rows"], x)
    end, _ = fold(st, ds)
    assert r in KC.key_rows(end, x)  # the fold keeps r
    both = np.union1d(ds[0]["keys"], ds[1]["keys"])
    mr, mc = R.join2(ds[0]["rows"], ds[0]["ctx"], ds[1]["rows"], ds[1]["ctx"], keys=both)
    one, _ = R.join2(st["rows"], st["ctx"], mr, mc, keys=both)
    assert r not in KC.key_rows(one, x)  # one join with the merged delta drops it


def test_remove_then_readd():
    st, ds, x, old, fresh = KC.remove_then_readd()
    assert every_row_in_its_keyset(ds) and len(old) >= 1
    assert KC.key_rows(fold(st, ds, 1)[0], x) == []          # delta 0 removed the key
    assert KC.key_rows(fold(st, ds, 4)[0], x) == []          # delta 3's covered row was dropped
    assert KC.key_rows(fold(st, ds)[0], x) == [fresh]        # delta 5's uncovered row stays


def test_shared_tuple():
    st, ds, tuples = KC.shared_tuple()
    assert every_row_in_its_keyset(ds) and len(ds) == 64
    held = [sum(t in KC.key_rows(d["rows"], t[0]) for d in ds) for t in tuples]
    assert held == [1, 2, 64]
    end, _ = fold(st, ds)
    for t in tuples:
        assert KC.key_rows(end, t[0]).count(t) == 1 and t not in KC.key_rows(st["rows"], t[0])


def test_empty_key():
    st, ds, z, L = KC.empty_key()
    assert len(ds) == 64 and all(z in d["keys"] for d in ds)
    assert all(KC.key_rows(d["rows"], z) == [] for d in ds) and KC.key_rows(st["rows"], z) == []
    end, _ = fold(st, ds)
    assert KC.key_rows(end, z) == []
    assert np.array_equal(R.store_diff(st["rows"], end), np.array([L], np.uint64))


def test_hazard():
    st, ds, h, want = KC.hazard()
    assert every_row_in_its_keyset(ds)
    union = np.unique(np.concatenate([d["keys"] for d in ds]))
    assert len(union) > 512
    end, _ = fold(st, ds)
    old = KC.key_rows(st["rows"], h)
    assert KC.key_rows(end, h) == want and len(old) == 3
    assert want[0] < old[0] and want[1:] == old[:2]          # [X, Y, Z] -> [D, X, Y], D < X
    assert np.array_equal(counts(st["rows"], union), counts(end, union))  # no key's count changes
    assert np.array_equal(R.store_diff(st["rows"], end), np.array([h], np.uint64))


def test_row_limits():
    for n_state, n_cand in ((64, 2), (65, 2), (3, 64), (3, 65)):
        st, ds, b = KC.row_limits(n_state, n_cand)
        assert every_row_in_its_keyset(ds)
        assert len(KC.key_rows(st["rows"], b)) == n_state
        cand = {r for d in ds for r in KC.key_rows(d["rows"], b)}
        assert len(cand) == n_cand and max(len(KC.key_rows(d["rows"], b)) for d in ds) <= 64
        end, _ = fold(st, ds)
        assert len(KC.key_rows(end, b)) == n_state - 1 + n_cand  # the first state row goes, every new row stays


def test_rows_in_one_delta():
    for n in (64, 65):
        st, ds, b = KC.rows_in_one_delta(n)
        assert every_row_in_its_keyset(ds)
        assert [len(KC.key_rows(d["rows"], b)) for d in ds] == [0, n] and KC.key_rows(st["rows"], b) == []
        assert len(KC.key_rows(fold(st, ds)[0], b)) == n
