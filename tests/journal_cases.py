"""Shared by the journal tests (test_storage_journal.py on the CPU, test_gpu_replace_keysets.py
and test_gpu_storage_journal.py on the device): small generators of SoA states, peer deltas
and journal records, and the per-key comparison of two states in numpy.  No test here."""
import numpy as np

from delta_crdt_ex_amd.interning import splitmix64_np
from delta_crdt_ex_amd.workloads import VV, sort_rows

DTYPES = (np.uint64, np.uint64, np.int64, np.uint32, np.uint64)


def empty_rows():
    return tuple(np.zeros(0, dt) for dt in DTYPES)


def key_space(n, seed):
    """n distinct hashed key ids, ascending (what Universe.key gives: uniform u64)."""
    return np.sort(splitmix64_np(np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed << 32)))


def rows_for(rng, keys, node, counter, lo=1, hi=3, p_none=0.0):
    """A store holding lo..hi rows of each of `keys` (none with probability p_none), every row
    a fresh dot of `node` from `counter` on.  Returns (rows in store order, next counter)."""
    ks, vs, ts, cs = [], [], [], []
    for k in keys:
        if rng.random() < p_none:
            continue
        for _ in range(int(rng.integers(lo, hi + 1))):
            ks.append(k)
            vs.append(int(rng.integers(0, 1 << 20)) + (1 << 62))
            ts.append(int(rng.integers(-(1 << 40), 1 << 40)))
            cs.append(counter)
            counter += 1
    rows = sort_rows(np.array(ks, np.uint64), np.array(vs, np.uint64), np.array(ts, np.int64),
                     np.full(len(ks), node, np.uint32), np.array(cs, np.uint64))
    return rows, counter


def take(rows, keys):
    m = np.isin(rows[0], np.asarray(keys, np.uint64))
    return tuple(c[m] for c in rows)


def rows_equal(a, b):
    return all(len(x) == len(y) and np.array_equal(x, y) for x, y in zip(a, b))


def changed_keys(old, new, keys):
    """The keys of `keys` (ascending) whose rows differ between two stores, by comparing each
    key's row slices."""
    out = []
    for k in np.asarray(keys, np.uint64):
        a0, a1 = np.searchsorted(old[0], k, "left"), np.searchsorted(old[0], k, "right")
        b0, b1 = np.searchsorted(new[0], k, "left"), np.searchsorted(new[0], k, "right")
        if a1 - a0 != b1 - b0 or any(not np.array_equal(x[a0:a1], y[b0:b1]) for x, y in zip(old, new)):
            out.append(k)
    return np.array(out, np.uint64)


def record(keys, rows, seq=0, ctx=None, root=None):
    """A journal record as storage.read_journal returns them."""
    keys = np.asarray(keys, np.uint64)
    return {"sequence_number": seq, "root": root, "keys": keys, "rows": rows, "terms": None,
            "ctx": ctx if ctx is not None else (VV, np.zeros(0, np.uint32), np.zeros(0, np.uint64))}


def naive_replay(rows, records):
    """Record after record through a dict of each key's rows: the semantics restated."""
    d = {}
    for r in zip(*[c.tolist() for c in rows]):
        d.setdefault(r[0], []).append(r)
    for rec in records:
        mine = {}
        for r in zip(*[c.tolist() for c in rec["rows"]]):
            mine.setdefault(r[0], []).append(r)
        for k in rec["keys"].tolist():
            if k in mine:
                d[k] = mine[k]
            else:
                d.pop(k, None)
    flat = [r for k in sorted(d) for r in d[k]]
    return tuple(np.array([r[i] for r in flat], dt) for i, dt in enumerate(DTYPES))
