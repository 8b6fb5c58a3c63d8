"""Crafted batches for dg_join_deltas_keyed (the fold of k keyed deltas, a thread per union
key): each is built so that one property of the fold's rule decides the result, and
tests/test_keyed_fold_cases.py proves with the C oracle that it does -- so a GPU pass on a
case means the kernel got that property right.  Every delta row's key is in its own delta's
keyset (the shape the keyed call serves).  Test data only (numpy)."""
import numpy as np

from kfold_cases import random_fold

VV = 0
V0 = 1 << 62  # value ids of the crafted rows (random_fold's are V0 + 0..3)


def rows_from(tuples):
    """[(key, val, ts, node, cnt)] -> the five sorted columns"""
    if not tuples:
        return (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint32),
                np.zeros(0, np.uint64))
    cols = tuple(np.array(x, dtype=t) for x, t in
                 zip(zip(*tuples), (np.uint64, np.uint64, np.int64, np.uint32, np.uint64)))
    o = np.lexsort((cols[4], cols[3], cols[2], cols[1], cols[0]))
    return tuple(np.ascontiguousarray(x[o]) for x in cols)


def with_rows(rows, tuples):
    """rows plus the tuples, sorted"""
    extra = rows_from(tuples)
    cols = tuple(np.concatenate([a, b]) for a, b in zip(rows, extra))
    o = np.lexsort((cols[4], cols[3], cols[2], cols[1], cols[0]))
    return tuple(np.ascontiguousarray(x[o]) for x in cols)


def vv(entries):
    """{node: counter} -> a version vector"""
    nodes = sorted(entries)
    return (VV, np.array(nodes, np.uint32), np.array([entries[n] for n in nodes], np.uint64))


def delta(tuples, ctx, keys):
    return {"rows": rows_from(tuples), "ctx": vv(ctx), "keys": np.unique(np.array(keys, np.uint64))}


def key_rows(rows, x):
    m = rows[0] == np.uint64(x)
    return [tuple(int(c[i]) for c in rows) for i in np.flatnonzero(m)]


def base():
    """3000 hashed keys of 1-3 rows, nodes 0..3 (the crafted rows use nodes >= 900)"""
    st, _ = random_fold(7, n_keys=3000, k=0, n_nodes=4)
    return st, np.unique(st["rows"][0])


def absent_key(keys, i):
    """a key the state does not hold"""
    x = np.uint64(0x0123456789ABCDEF + 7919 * i)
    assert x not in keys
    return int(x)


def net_no_change():
    """K gets a row from delta 0 that delta 1 removes again; L is really updated."""
    st, keys = base()
    K, L = int(keys[100]), int(keys[2000])
    d0 = delta([(K, V0, 50, 900, 1), (L, V0 + 1, 50, 900, 2)], {900: 2}, [K, L])
    d1 = delta([], {900: 1}, [K])
    return st, [d0, d1], K, L


def order_dependence():
    """Row r of key x is in the state and in d1; c0 covers dot(r), d0 lacks r and x is not in
    K0: the fold keeps r, one join with the merged delta does not."""
    st, keys = base()
    x, y = int(keys[500]), int(keys[1500])
    r = key_rows(st["rows"], x)[0]
    d0 = delta([(y, V0 + 2, 60, 900, 1)], {r[3]: r[4], 900: 1}, [y])
    d1 = delta([r], {r[3]: r[4]}, [x])
    return st, [d0, d1], x, r


def remove_then_readd():
    """Delta 0 removes key x's rows; delta 3 re-adds one of them, whose dot the context covers
    by then (dropped); delta 5 re-adds a row with an uncovered dot (kept).  Deltas 1, 2, 4
    touch another key."""
    st, keys = base()
    x, y = int(keys[700]), int(keys[701])
    old = key_rows(st["rows"], x)
    cover = {}
    for r in old:
        cover[r[3]] = max(cover.get(r[3], 0), r[4])
    fresh = (x, V0 + 3, 70, 901, 5)
    ds = [delta([], cover, [x]),
          delta([], {}, [y]),
          delta([], {}, [y]),
          delta([old[0]], {}, [x]),
          delta([], {}, [y]),
          delta([fresh], {901: 5}, [x])]
    return st, ds, x, old, fresh


def shared_tuple():
    """The same new tuple held by 1, 2 and all 64 deltas (keys x1, x2, x3)."""
    st, keys = base()
    x1, x2, x3 = int(keys[10]), int(keys[1000]), int(keys[2300])
    t1, t2, t3 = (x1, V0, 80, 903, 1), (x2, V0, 80, 904, 1), (x3, V0, 80, 902, 1)
    ds = []
    for i in range(64):
        rows, ctx, ks = [t3], {902: 1}, [x3]
        if i == 10:
            rows, ctx, ks = rows + [t1], {**ctx, 903: 1}, ks + [x1]
        if i in (20, 40):
            rows, ctx, ks = rows + [t2], {**ctx, 904: 1}, ks + [x2]
        ds.append(delta(rows, ctx, ks))
    return st, ds, (t1, t2, t3)


def empty_key():
    """A key in all 64 keysets with no rows anywhere (and one key that really changes)."""
    st, keys = base()
    z, L = absent_key(keys, 1), int(keys[42])
    ds = [delta([], {902: 1}, [z]) for _ in range(64)]
    ds[0] = delta([(L, V0, 90, 902, 1)], {902: 1}, [z, L])
    return st, ds, z, L


def hazard():
    """Key h goes [X, Y, Z] -> [D, X, Y] with D < X: delta 0 removes Z, delta 1 adds D.  Every
    other key of the two keysets (600 of them) keeps its rows, so no key's row count changes
    -- and an in-place write of h's rows in tuple order would overwrite X before reading it."""
    st, keys = base()
    h = absent_key(keys, 2)
    X, Y, Z, D = (h, V0 + 10, 5, 907, 1), (h, V0 + 20, 5, 907, 2), (h, V0 + 30, 5, 905, 1), (h, V0 + 5, 5, 906, 1)
    st = {"rows": with_rows(st["rows"], [X, Y, Z]), "ctx": st["ctx"]}
    d0 = delta([], {905: 1}, [h] + [int(k) for k in keys[0:600:2]])
    d1 = delta([D], {906: 1}, [h] + [int(k) for k in keys[1:600:2]])
    return st, [d0, d1], h, [D, X, Y]


def row_limits(n_state, n_cand):
    """One key with n_state state rows, and n_cand distinct new delta rows of it spread over
    two deltas (the first also removes the key's first state row)."""
    st, keys = base()
    b = absent_key(keys, 3)
    srows = [(b, V0 + 100 + i, 5, 908, 1 + i) for i in range(n_state)]
    half = n_cand // 2
    cand = [(b, V0 + 1000 + i, 6, 909 if i < half else 910, 1 + i) for i in range(n_cand)]
    st = {"rows": with_rows(st["rows"], srows), "ctx": st["ctx"]}
    d0 = delta(cand[:half], {908: 1, 909: half}, [b])
    d1 = delta(cand[half:], {910: n_cand}, [b])
    return st, [d0, d1], b


def rows_in_one_delta(n):
    """One key whose n new rows all sit in ONE of two deltas (the other names the key and holds
    nothing): the per-delta limit of 64 rows of a key, apart from the limit on distinct rows."""
    st, keys = base()
    b = absent_key(keys, 4)
    new = [(b, V0 + 2000 + i, 7, 911, 1 + i) for i in range(n)]
    return st, [delta([], {}, [b]), delta(new, {911: n}, [b])], b
