"""A CPU model of the one-pass fold's bucket plan (csrc/kfold.hip, kfold_pass in
csrc/api_fold.hip), and inputs built to reach its seams (helper module: no tests).

The fold cuts the key space into T equal buckets sized by means, stages every bucket in
fixed LDS arrays, flags KF_OVERFLOW when one does not fit and retries once with 8 T.  From
outside the library only "folded in one pass" (the strict engine answers) or "refused" (it
raises) shows, so WHICH path an input takes -- first attempt, retry, which overflow site,
whether a thread stages a second item -- is decided here, by a line-by-line restatement of
the host's and the kernel's decisions.  tests/test_kfold_plan.py pins the constants below
to csrc/dg_launch.h and asserts, for every input of tests/test_gpu_kfold_seams.py, that the
model sends it down the path the GPU test is for."""
import functools

import numpy as np

import skew
from delta_crdt_ex_amd.interning import splitmix64_np
from kfold_cases import DOTS, VV, mutation_fold, random_fold
from oracle import ref as R

# ---------------------------------------------------------------- the constants (one table)
# csrc/dg_launch.h (checked by test_kfold_plan.py::test_constants_match_the_header); NSUB is
# csrc/kfold.hip's DG_KFOLD_NSUB.
CONST = {
    "DG_KFOLD_SCALE": 0, "DG_KFOLD_BLOCK": 1024,
    "KFOLD_CAP_S": 1024, "KFOLD_CAP_D": 512, "KFOLD_CAP_M": 512,
    "KFOLD_MEAN_S": 800, "KFOLD_MEAN_D": 400, "KFOLD_MEAN_M": 800, "KFOLD_MEAN_U": 1200,
    "KFOLD_MAX_K": 64, "KNT": 1024, "KF_CNT_LIMIT": (1 << 48) - 1,
    "DG_KFOLD_NSUB": 1024,
}
KB = CONST["DG_KFOLD_BLOCK"]
CS, CD, CM = CONST["KFOLD_CAP_S"], CONST["KFOLD_CAP_D"], CONST["KFOLD_CAP_M"]
CU = CD + CM        # items after the keyset fold
CUL = CD + 2 * CM   # items staged
MEAN_S, MEAN_D, MEAN_M, MEAN_U = (CONST["KFOLD_MEAN_" + x] for x in "SDMU")
MAX_K, KNT, CNT_LIMIT, NSUB = (CONST["KFOLD_MAX_K"], CONST["KNT"], CONST["KF_CNT_LIMIT"],
                               CONST["DG_KFOLD_NSUB"])
TOP = (1 << 64) - 1
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------- the model

def mulhi(a, b):
    """__umul64hi(a, b) for a uint64 array a and an int b < 2^64."""
    a = np.asarray(a, np.uint64)
    s = np.uint64(32)
    ah, al = a >> s, a & M32
    bh, bl = np.uint64(b >> 32), np.uint64(b & 0xFFFFFFFF)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> s) + (lh & M32) + (hl & M32)
    return hh + (lh >> s) + (hl >> s) + (mid >> s)


def bucket_of(keys, T):
    return mulhi(keys, T).astype(np.int64)


def sub_of(keys, T):
    """(bucket, sub-bucket) of every key: kfold.hip's sub_of is the second, per bucket."""
    g = mulhi(keys, T * NSUB).astype(np.int64)
    return g // NSUB, g % NSUB


def _ceil_div(a, b):
    return (a + b - 1) // b


def _is_full(d):
    return d["keys"] is None


def t0(state, deltas):
    """kfold_pass's first bucket count."""
    n_s = len(state["rows"][0])
    rows = sum(len(d["rows"][0]) for d in deltas)
    keys = sum(0 if _is_full(d) else len(d["keys"]) for d in deltas)
    return max(_ceil_div(n_s, MEAN_S), _ceil_div(rows, MEAN_D), _ceil_div(keys, MEAN_M),
               _ceil_div(rows + keys, MEAN_U), 1)


def _kept(d):
    """The keyset entries of a delta that has no row of their key."""
    if _is_full(d):
        return np.zeros(0, np.uint64)
    return d["keys"][~np.isin(d["keys"], d["rows"][0])]


def plan(state, deltas, T):
    """Per bucket t = (key T) >> 64 of one kfold_kernel launch over <= 64 deltas: a list of
    dicts with
      nS, nD, nM     state rows, delta rows, keyset entries as the kernel counts them (every
                     run's length bounded by CUL + 1, as `len` is)
      n_keep         keyset entries whose own delta has no row of that key
      first, second  the two overflow predicates as kfold_kernel writes them (the second is
                     only reached, with the counts intact, when the first did not fire)
      why            the first predicate's terms that hold: letters of "SDUM" (state rows,
                     delta rows, staged items, staged keyset entries)
      max_sub        the largest number of items (delta rows + kept entries) in one of the
                     NSUB sub-buckets; max_sub_s the same for state rows
      q2             some thread stages a second item (index >= KB)"""
    assert 1 <= len(deltas) <= MAX_K
    n_s = np.bincount(bucket_of(state["rows"][0], T), minlength=T)
    n_d = np.zeros(T, np.int64)
    n_m = np.zeros(T, np.int64)
    n_keep = np.zeros(T, np.int64)
    for d in deltas:
        n_d += np.minimum(np.bincount(bucket_of(d["rows"][0], T), minlength=T), CUL + 1)
        if not _is_full(d):
            n_m += np.minimum(np.bincount(bucket_of(d["keys"], T), minlength=T), CUL + 1)
            n_keep += np.bincount(bucket_of(_kept(d), T), minlength=T)
    items = np.concatenate([d["rows"][0] for d in deltas] + [_kept(d) for d in deltas])

    def max_sub(keys):
        out = np.zeros(T, np.int64)
        if len(keys):
            b, s = sub_of(keys, T)
            u, c = np.unique(b * NSUB + s, return_counts=True)
            np.maximum.at(out, u // NSUB, c)
        return out

    ms_u, ms_s = max_sub(items), max_sub(state["rows"][0])
    out = []
    for t in range(T):
        nS, nD, nU = int(n_s[t]), int(n_d[t]), int(n_d[t] + n_m[t])
        terms = (("S", nS > CS), ("D", nD > CD), ("U", nU > CUL), ("M", nU - nD > CUL - CD))
        first = nS > CS or nD > CD or nU > CUL or nU - nD > CUL - CD
        second = (not first) and nD + int(n_keep[t]) > CU
        out.append(dict(nS=nS, nD=nD, nM=nU - nD, n_keep=int(n_keep[t]), first=first,
                        why="".join(n for n, b in terms if b),
                        second=second, max_sub=int(ms_u[t]), max_sub_s=int(ms_s[t]),
                        q2=(not first) and nU > KB))
    return out


def host_refusal(state, deltas):
    """Why kfold_pass / kfold_prep hand this pass to the step-by-step fold before any bucket
    is looked at (None: they do not)."""
    if not 1 <= len(deltas) <= MAX_K:
        return "delta count"
    if state["ctx"][0] != VV:
        return "state context is a dot set"
    if len(state["ctx"][1]) and int(np.max(state["ctx"][1])) >= KNT:
        return "node >= KNT in the state's context"
    for d in deltas:
        kind, node, cnt = d["ctx"]
        if len(node) and int(np.max(node)) >= KNT:
            return "node >= KNT in a delta context"
        if kind == DOTS and len(cnt) and int(np.max(cnt)) >= CNT_LIMIT:
            return "dot counter >= KF_CNT_LIMIT"
    return None


def trace_pass(state, deltas):
    """One kfold_pass: dict(verdict, host, T0, attempts=[dict(T, first=[buckets],
    second=[buckets], q2=[buckets])]).  verdict: "first" (the fold at T0 stands), "retry"
    (T0 overflowed, 8 T0 stands) or "refuse" (the caller folds step by step)."""
    host = host_refusal(state, deltas)
    if host is not None:
        return dict(verdict="refuse", host=host, T0=None, attempts=[])
    T0 = t0(state, deltas)
    attempts = []
    for a in range(2):
        T = T0 << (3 * a)
        p = plan(state, deltas, T)
        attempts.append(dict(T=T, first=[t for t in range(T) if p[t]["first"]],
                             second=[t for t in range(T) if p[t]["second"]],
                             q2=[t for t in range(T) if p[t]["q2"]]))
        if not attempts[-1]["first"] and not attempts[-1]["second"]:
            return dict(verdict=("first", "retry")[a], host=None, T0=T0, attempts=attempts)
    return dict(verdict="refuse", host=None, T0=T0, attempts=attempts)


def traces(state, deltas):
    """dg_apply_deltas' passes of up to 64 deltas; a later pass folds into the earlier
    passes' result (the oracle's), and none runs after a refused one."""
    out = []
    st = state
    for i0 in range(0, len(deltas), MAX_K):
        ds = deltas[i0:i0 + MAX_K]
        out.append(trace_pass(st, ds))
        if out[-1]["verdict"] == "refuse":
            break
        if i0 + MAX_K < len(deltas):
            rows, ctx = R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds],
                                       [d["ctx"] for d in ds], [d["keys"] for d in ds])
            st = {"rows": rows, "ctx": ctx}
    return out


def verdict(state, deltas):
    """ "refuse" when any pass refuses (the strict engine raises, the default one folds all
    the deltas step by step), else "retry" when any pass retried, else "first"."""
    vs = [t["verdict"] for t in traces(state, deltas)]
    return "refuse" if "refuse" in vs else "retry" if "retry" in vs else "first"


# the hash set of the dot-set contexts' dots (kfold.hip dset_key / dset_slot, kfold_pass dset_n)
def dset_key(i, node, cnt):
    return ((cnt << 16) | (node << 6) | i) & TOP


def dset_slot(key, mask):
    x = (key * 0x9E3779B97F4A7C15) & TOP
    return (x ^ (x >> 29)) & mask


def dset_size(deltas):
    n = sum(len(d["ctx"][1]) for d in deltas if d["ctx"][0] == DOTS)
    size = 1024
    while size < 2 * n:
        size <<= 1
    return size


def dset_table(deltas, reverse=False):
    """The table kfold_dset_kernel builds when the dots arrive in flat order (or in the
    reverse of it: the device's order is not fixed)."""
    size = dset_size(deltas)
    tab = [None] * size
    ks = [dset_key(i, int(nd), int(c)) for i, d in enumerate(deltas) if d["ctx"][0] == DOTS
          for nd, c in zip(d["ctx"][1], d["ctx"][2]) if nd < KNT and c < CNT_LIMIT]
    for key in (reversed(ks) if reverse else ks):
        h = dset_slot(key, size - 1)
        while tab[h] is not None and tab[h] != key:
            h = (h + 1) & (size - 1)
        tab[h] = key
    return tab


def dset_probe(tab, i, node, cnt):
    """covers()' probe of dot (node, cnt) in c_i: (found, the slots read)."""
    key = dset_key(i, node, cnt)
    h = dset_slot(key, len(tab) - 1)
    seen = []
    while True:
        seen.append(h)
        if tab[h] == key:
            return True, seen
        if tab[h] is None:
            return False, seen
        h = (h + 1) & (len(tab) - 1)


# ---------------------------------------------------------------- row helpers

def _sel(rows, m):
    return tuple(np.ascontiguousarray(c[m]) for c in rows)


def _sorted_unique(rows):
    o = np.lexsort((rows[4], rows[3], rows[2], rows[1], rows[0]))
    rows = tuple(c[o] for c in rows)
    if len(o) > 1:
        same = np.ones(len(o) - 1, bool)
        for c in rows:
            same &= c[1:] == c[:-1]
        rows = _sel(rows, np.concatenate([[True], ~same]))
    return tuple(np.ascontiguousarray(c) for c in rows)


def merge_rows(*sets):
    return _sorted_unique(tuple(np.concatenate([s[j] for s in sets]) for j in range(5)))


def pool(seed, keys, k, rows_per_key=2, **kw):
    """random_fold's row pool on the given keys (1..rows_per_key tuples per key, unique
    dots), its state context and k delta contexts: (rows, ctx, [ctx_i])."""
    st, ds = random_fold(seed, keys=keys, k=k, rows_per_key=rows_per_key, p_state=1.0, p_keys=0.0,
                         p_outside=0.0, **kw)
    return st["rows"], st["ctx"], [d["ctx"] for d in ds]


def _distinct(rng, lo, hi, n):
    """n distinct keys uniform in [lo, hi), sorted."""
    u = skew._cut(lambda m: rng.integers(lo, hi, m, dtype=np.uint64), n)
    return np.sort(rng.choice(u, n, replace=False))


def fold_keys(fold):
    st, ds = fold
    return np.unique(np.concatenate([st["rows"][0]] + [d["rows"][0] for d in ds] +
                                    [d["keys"] for d in ds if d["keys"] is not None]))


def rekeyed(fold, key_set):
    """The fold with the i-th smallest of its distinct keys (rows' and keysets') replaced by
    key_set[i].  The map is strictly increasing: every store and keyset stays sorted and
    unique, and the oracle's result is the same map of its result on the original."""
    st, ds = fold
    old = fold_keys(fold)
    key_set = np.asarray(key_set, np.uint64)
    assert len(key_set) == len(old) and bool(np.all(key_set[1:] > key_set[:-1]))

    def remap(keys):
        return key_set[np.searchsorted(old, keys)]

    def rows(r):
        return (remap(r[0]),) + tuple(r[1:])

    return ({**st, "rows": rows(st["rows"])},
            [{**d, "rows": rows(d["rows"]), "keys": None if d["keys"] is None else remap(d["keys"])}
             for d in ds])


def dense_part(rng, n, f, w):
    """A fraction f of n keys uniform in [0, 2^64 / w), the rest uniform: a dense w-th."""
    nd = int(round(f * n))
    low = _distinct(rng, 0, (1 << 64) // w, nd)
    rest = skew._cut(lambda m: np.setdiff1d(rng.integers(0, 1 << 64, m, dtype=np.uint64), low), n - nd)
    return np.sort(np.concatenate([low, rng.choice(rest, n - nd, replace=False)]))


KEY_SETS = dict(skew.GENERATORS,
                dense_half_16th=lambda rng, n: dense_part(rng, n, 0.5, 16),
                dense_third_8th=lambda rng, n: dense_part(rng, n, 0.3, 8))


@functools.lru_cache(maxsize=None)
def _skewed(name, seed, n_keys, k, kw):
    fold = random_fold(seed, n_keys=n_keys, k=k, **dict(kw))
    ks = KEY_SETS[name](np.random.default_rng(seed + 1000), len(fold_keys(fold)))
    return rekeyed(fold, ks)


def skewed_fold(name, seed, n_keys, k, **kw):
    """random_fold(seed, n_keys, k, **kw) rekeyed to a key set of the named generator."""
    return _skewed(name, seed, n_keys, k, tuple(sorted(kw.items())))


# The rekeyed folds of test_gpu_kfold_seams.py::test_rekeyed and what the model says of them
# (test_kfold_plan.py::test_rekeyed_reach asserts the verdicts and the overflow sites).
# Big key sets of the skew generators put thousands of rows into bucket 0 at any T: refused.
# Small ones fit one bucket (T0 = 1) whatever the keys are: the skew is then INSIDE the bucket.
SKEW_CASES = {
    "uniform":               ("uniform", 200, 6000, 6, {}, "first"),
    "geometric":             ("geometric", 201, 6000, 6, {}, "refuse"),
    "two_clusters":          ("two_clusters", 202, 6000, 6, {}, "refuse"),
    "dense_plus_max":        ("dense_plus_max", 203, 6000, 6, {}, "refuse"),
    "geometric small":       ("geometric", 204, 450, 6, dict(p_keys=0.1), "first"),
    "two_clusters small":    ("two_clusters", 205, 450, 8, dict(p_keys=0.15), "first"),
    "dense_plus_max small":  ("dense_plus_max", 206, 450, 6, dict(p_keys=0.1), "first"),
    "dense_half_16th":       ("dense_half_16th", 207, 6000, 6, {}, "retry"),
    "dense_third_8th":       ("dense_third_8th", 208, 6000, 6, {}, "retry"),
    "dense_half_16th dots":  ("dense_half_16th", 209, 5000, 8, dict(delta_dots=True), "retry"),
    "dense_third_8th full":  ("dense_third_8th", 210, 5000, 8, dict(p_full=0.3), "retry"),
    "two_clusters dots+full": ("two_clusters", 211, 450, 8, dict(p_keys=0.15, delta_dots=True,
                                                                p_full=0.5), "first"),
}


def skew_case(name):
    gen, seed, n_keys, k, kw, _ = SKEW_CASES[name]
    return skewed_fold(gen, seed, n_keys, k, **kw)


# ---------------------------------------------------------------- at the capacities
OVERS = ("S", "D", "M", "keep")
# what bucket 0 holds: state rows, delta rows, delta rows whose key is in their own delta's
# keyset (their entry folds into them), keyset entries of keys their delta has no row of
_CAPACITY = {None: (CS, CD, CD, CM), "S": (CS + 1, CD, CD, CM), "D": (CS, CD + 1, CD, CM - 1),
             "M": (CS, CD - 1, CD - 1, CM + 2), "keep": (CS, CD, CD - 1, CM + 1)}


@functools.lru_cache(maxsize=None)
def at_capacity(over=None, spread=False, layout="one", seed=7):
    """A fold of two buckets (T0 = 2 by all four terms of kfold_pass's formula) whose
    bucket 0 sits exactly AT every capacity: 1024 state rows, 512 delta rows and 1024 keyset
    entries, of which 512 fold into their delta's rows and 512 are kept -- 1536 staged items
    (512 of them second items of a thread) and 1024 after the keyset fold.  Bucket 1 holds
    about 100 state rows, 8 delta rows and 6 keyset entries.

    over: one element more in one dimension, the others at or below their capacity:
      "S"     1025 state rows
      "D"     513 delta rows (1023 keyset entries: 1536 staged)
      "M"     1025 keyset entries (511 delta rows: 1536 staged)
      "keep"  512 delta rows of which 511 take their entry, 513 kept entries: 1024 keyset
              entries, 1536 staged, every first-site term at its capacity, and 1025 items
              after the keyset fold -- the second overflow site alone.
    There is no "U" (nU > CUL alone): CUL = CD + 2 CM is the sum of the row capacity and the
    entry capacity, so nU > CUL implies nD > CD or nU - nD > CUL - CD.

    spread=False: bucket 0's keys lie below 2^60, so at T = 16 bucket 0 holds the same
    elements and the retry overflows as well; spread=True: they are uniform in [0, 2^63) and
    8 T0 fits.  layout: "one" delta holds all of it, or "many" = 64 deltas of 8 rows and 16
    entries each (the extra element in delta 63)."""
    n_s, n_d, n_fold, n_kept = _CAPACITY[over]
    k = {"one": 1, "many": 64}[layout]
    rng = np.random.default_rng(1000 + seed)
    n_c = 400  # keys no delta touches
    hi0 = (1 << 63) if spread else (1 << 60)
    k0 = rng.permutation(_distinct(rng, 1, hi0, n_d + n_kept + n_c))
    a_keys, b_keys = np.sort(k0[:n_d]), np.sort(k0[n_d:n_d + n_kept])
    k1 = rng.permutation(_distinct(rng, 1 << 63, 1 << 64, 70))
    # bucket 1: 8 rows, 3 of them with their key in the keyset, 3 kept entries
    a1, b1 = np.sort(k1[:8]), np.sort(k1[8:11])
    f1 = a1[:3]
    prow, ctx, dctx = pool(seed, np.concatenate([k0, k1]), k)
    in0 = np.flatnonzero(prow[0] < np.uint64(1 << 63))
    in1 = np.flatnonzero(prow[0] >= np.uint64(1 << 63))
    assert len(in0) >= n_s
    state = {"rows": _sel(prow, np.sort(np.concatenate([rng.choice(in0, n_s, replace=False), in1]))),
             "ctx": ctx}
    first_row = dict(zip(*np.unique(prow[0], return_index=True)))  # a key's first pool row

    def owner(j):  # the j-th key of a class goes to delta 63 - j % 64: the extras to delta 63
        return 0 if k == 1 else 63 - j % 64

    didx = [[] for _ in range(k)]
    dkeys = [[] for _ in range(k)]
    for j, key in enumerate(a_keys):
        didx[owner(j)].append(first_row[key])
        if j >= n_d - n_fold:  # (the first n_d - n_fold rows: carried, not in the keyset)
            dkeys[owner(j)].append(key)
    for j, key in enumerate(b_keys):
        dkeys[owner(j)].append(key)
    for j, key in enumerate(a1):
        didx[0 if k == 1 else j].append(first_row[key])
    for j, key in enumerate(f1):
        dkeys[0 if k == 1 else j].append(key)
    for j, key in enumerate(b1):
        dkeys[0 if k == 1 else j + 3].append(key)
    deltas = [{"rows": _sel(prow, np.sort(np.array(didx[i], np.int64))), "ctx": dctx[i],
               "keys": np.sort(np.array(dkeys[i], np.uint64))} for i in range(k)]
    return state, deltas


# ---------------------------------------------------------------- skew inside a bucket

@functools.lru_cache(maxsize=None)
def one_sub_bucket(seed=80):
    """Consecutive integer keys 1..n: one bucket (T0 = 1) and ONE of its 1024 sub-buckets
    holds every state row and every item, so the rank loop and the sfirst fill walk the
    whole bucket."""
    return random_fold(seed, n_keys=520, k=6, rows_per_key=2, hashed=False, p_keys=0.12)


@functools.lru_cache(maxsize=None)
def one_key_bucket(seed=81, key=5):
    """ONE key: 1024 state rows and 512 delta rows of it over 16 deltas (T0 = 2: bucket 0 at
    its state and row capacities, bucket 1 empty).  Deltas 0, 4, 8, 12 are full-state joins,
    delta 1 has an empty keyset (its rows replace the key's), delta 9 has no rows and names
    the key (a removal), the others name the key.  Every walk over "the items of this key"
    spans the whole bucket."""
    rng = np.random.default_rng(2000 + seed)
    prow, ctx, dctx = pool(seed, np.arange(1, 1501, dtype=np.uint64), 16, rows_per_key=1)
    prow = _sorted_unique((np.full(len(prow[0]), key, np.uint64),) + tuple(prow[1:]))
    n = len(prow[0])
    state = {"rows": _sel(prow, np.sort(rng.choice(n, CS, replace=False))), "ctx": ctx}
    sizes = [0 if i == 9 else 34 for i in range(16)]
    sizes[0] += 1
    sizes[2] += 1
    assert sum(sizes) == CD
    deltas = []
    for i in range(16):
        ks = None if i % 4 == 0 else np.zeros(0, np.uint64) if i == 1 else np.array([key], np.uint64)
        deltas.append({"rows": _sel(prow, np.sort(rng.choice(n, sizes[i], replace=False))),
                       "ctx": dctx[i], "keys": ks})
    return state, deltas


END_KEYS = np.array([0, 1, TOP - 1, TOP], np.uint64)


@functools.lru_cache(maxsize=None)
def ends():
    """Keys 0, 1, 2^64 - 2 and 2^64 - 1 among hashed keys, each of the four present in the
    state, in some delta's rows and in some keyset (the first seed for which that holds)."""
    keys = np.concatenate([END_KEYS, splitmix64_np(np.arange(1, 1497, dtype=np.uint64))])
    for seed in range(300, 400):
        st, ds = random_fold(seed, keys=keys, k=6, rows_per_key=3, p_state=0.85, p_keys=0.3,
                             p_take=0.6)
        if ends_present(st, ds):
            return st, ds
    raise AssertionError("no seed puts the end keys everywhere")


def ends_present(st, ds):
    return all(np.isin(END_KEYS, c).all() for c in
               (st["rows"][0], np.concatenate([d["rows"][0] for d in ds]),
                np.concatenate([d["keys"] for d in ds])))


@functools.lru_cache(maxsize=None)
def all_runs_one_bucket(seed=82):
    """k = 64 and T0 = 1: all 128 runs (64 deltas' rows, 64 keysets) are non-empty in the one
    bucket, every delta with at least one row and one keyset entry that does not fold into
    a row -- delta 63 too.  The deltas draw their keys from 60 hot keys, so a key's K / R / M
    masks carry many bits, bit 63 among them."""
    rng = np.random.default_rng(3000 + seed)
    keys = splitmix64_np(np.arange(1, 481, dtype=np.uint64))
    prow, ctx, dctx = pool(seed, keys, 64)
    hot = keys[:60]
    head = np.concatenate([[True], prow[0][1:] != prow[0][:-1]])  # a key's first pool row
    state = {"rows": _sel(prow, rng.random(len(prow[0])) < 0.75), "ctx": ctx}
    deltas = []
    for i in range(64):
        mine = rng.choice(hot[1:], 6, replace=False)
        if i == 63:
            mine[0] = hot[0]  # hot[0]: delta 63 holds rows of it and delta 62 names it
        if i == 62:
            mine[3] = hot[0]
        rows = _sel(prow, np.isin(prow[0], mine[:3]) & (head | (rng.random(len(prow[0])) < 0.6)))
        # two of the row keys (the third's rows are carried) and three keys without rows
        deltas.append({"rows": rows, "ctx": dctx[i], "keys": np.sort(np.concatenate([mine[:2], mine[3:]]))})
    return state, deltas


@functools.lru_cache(maxsize=None)
def gaps(seed=83):
    """T0 = 8 by the delta rows.  The state sits in ONE narrow key range inside bucket 5, which
    no delta touches (state_start's 64-ary search ends inside one bucket; bucket 5 has state
    rows and no item, every other bucket items and no state row).  Delta 4 and its keyset
    hold keys only below 2^40 and above 2^64 - 2^40: its runs are empty in buckets 1..6, the
    fill's `for (; bb <= end; bb++)` loop over a long gap; delta 5 is empty with an empty
    keyset."""
    rng = np.random.default_rng(4000 + seed)
    lo5, hi5 = (5 << 64) // 8, (6 << 64) // 8
    h = splitmix64_np(np.arange(1, 2301, dtype=np.uint64))
    h = h[(h < np.uint64(lo5)) | (h >= np.uint64(hi5))]
    narrow = _distinct(rng, lo5 + (1 << 58), lo5 + (1 << 58) + (1 << 30), 500)
    low, high = _distinct(rng, 0, 1 << 40, 40), _distinct(rng, TOP - (1 << 40), TOP, 40)
    prow, ctx, dctx = pool(seed, np.concatenate([h, narrow, low, high]), 6, rows_per_key=3)
    in_narrow = np.isin(prow[0], narrow)
    state = {"rows": _sel(prow, in_narrow & (rng.random(len(prow[0])) < 0.9)), "ctx": ctx}
    deltas = []
    for i in range(4):
        kk = h[rng.random(len(h)) < 0.25]
        deltas.append({"rows": _sel(prow, np.isin(prow[0], kk) & (rng.random(len(prow[0])) < 0.7)),
                       "ctx": dctx[i], "keys": np.sort(kk[rng.random(len(kk)) < 0.8])})
    ends_ = np.concatenate([low, high])
    deltas.append({"rows": _sel(prow, np.isin(prow[0], ends_[::2])), "ctx": dctx[4],
                   "keys": np.sort(ends_[::3])})
    deltas.append({"rows": _sel(prow, np.zeros(len(prow[0]), bool)), "ctx": dctx[5],
                   "keys": np.zeros(0, np.uint64)})
    return state, deltas


@functools.lru_cache(maxsize=None)
def tiny_absent_keys(seed=84):
    """T0 = 1 (a state of ~120 rows, three small deltas); delta 0's keyset names only keys
    that neither the state nor any delta holds, delta 1's only keys of the state."""
    st, ds = random_fold(seed, n_keys=100, k=3, p_keys=0.2)
    present = fold_keys((st, ds))
    absent = np.setdiff1d(present[present != np.uint64(TOP)] + np.uint64(1), present)[:40]
    ds = [dict(ds[0], keys=absent), dict(ds[1], keys=np.unique(st["rows"][0])[::3])] + ds[2:]
    return st, ds


# ---------------------------------------------------------------- dot-set edges
DOT_CASES = {"counter 2^48-2": "taken", "counter 2^48-1": "refuse", "node 1023": "taken",
             "node 1024": "refuse", "probe wrap": "taken"}
WRAP_DELTA, WRAP_NODE = 1, 1000


def wrap_counters(n=3, mask=1023):
    """The first n counters whose dot (WRAP_NODE, counter) of delta WRAP_DELTA has its home
    in the LAST slot of a 1024-slot table."""
    out, c = [], 1
    while len(out) < n:
        if dset_slot(dset_key(WRAP_DELTA, WRAP_NODE, c), mask) == mask:
            out.append(c)
        c += 1
    return out


@functools.lru_cache(maxsize=None)
def dot_edges(case, seed=85):
    """Three mutation deltas (dot-set contexts, fewer than 512 dots: the 1024-slot table)
    against a VV state, with extra rows put on a key that delta 1 removes, and some of their
    dots put into delta 1's context:
      counter 2^48-2 / 2^48-1   a dot of node 7 with that counter, in the state and in c_1
                                (the first packs into a hash key, the second is
                                KF_CNT_LIMIT: the prep refuses), and a sibling one below
                                that c_1 does not hold
      node 1023 / 1024          the same with the node id at the VV tables' width
      probe wrap                three dots whose home is slot 1023, two of them in c_1:
                                one of the two sits in slot 0, and the lookup of the third
                                (absent) runs through 1023, 0, ... to an empty slot.
    Returns (state, deltas, dots): the extra rows' dots, [(node, counter, in c_1)]."""
    st, ds = mutation_fold(seed, n_keys=1500, k=3, ops=40)
    d1 = ds[WRAP_DELTA]
    removed = d1["keys"][~np.isin(d1["keys"], d1["rows"][0]) & np.isin(d1["keys"], st["rows"][0])]
    assert len(removed)
    key = int(removed[0])
    big = (1 << 48) - 2
    dots = {"counter 2^48-2": [(7, big, True), (7, big - 1, False)],
            "counter 2^48-1": [(7, big + 1, True), (7, big, False)],
            "node 1023": [(1023, 9, True), (1023, 8, False)],
            "node 1024": [(1024, 9, True), (1024, 8, False)]}.get(case)
    if dots is None:
        a, b, c = wrap_counters()
        dots = [(WRAP_NODE, a, True), (WRAP_NODE, b, True), (WRAP_NODE, c, False)]
    n = len(dots)
    extra = (np.full(n, key, np.uint64), np.uint64(1 << 62) + np.arange(n, dtype=np.uint64),
             np.arange(n, dtype=np.int64), np.array([x[0] for x in dots], np.uint32),
             np.array([x[1] for x in dots], np.uint64))
    st = {"rows": merge_rows(st["rows"], extra), "ctx": st["ctx"]}
    cn = np.concatenate([d1["ctx"][1], np.array([x[0] for x in dots if x[2]], np.uint32)])
    cc = np.concatenate([d1["ctx"][2], np.array([x[1] for x in dots if x[2]], np.uint64)])
    o = np.lexsort((cc, cn))
    ds = list(ds)
    ds[WRAP_DELTA] = dict(d1, ctx=(DOTS, np.ascontiguousarray(cn[o]), np.ascontiguousarray(cc[o])))
    return st, ds, dots


# ---------------------------------------------------------------- 70 deltas: two passes

def _with_absent(d, keys):
    return dict(d, keys=np.union1d(d["keys"], keys))


@functools.lru_cache(maxsize=None)
def two_pass(case, seed=86):
    """random_fold(n_keys=3000, k=70): a pass of 64 deltas and one of 6, with
      "second prep fails"      node 1024 in delta 66's context: pass 1 folds, pass 2 is refused
                               by the prep
      "second overflows twice" delta 65's keyset also names 1100 absent keys below 2^40:
                               more than 1024 keyset entries in bucket 0 at T0 and at 8 T0
      "first retries"          delta 3's keyset also names 1100 absent keys spread over a
                               quarter of bucket 1 of pass 1's T0: over 1024 entries there,
                               half of that in each of two buckets at 8 T0; pass 2 fits at
                               once."""
    st, ds = random_fold(seed, n_keys=3000, k=70, p_keys=0.02)
    ds = list(ds)
    rng = np.random.default_rng(5000 + seed)
    present = fold_keys((st, ds))
    if case == "second prep fails":
        kind, node, cnt = ds[66]["ctx"]
        ds[66] = dict(ds[66], ctx=(kind, np.append(node, np.uint32(1024)), np.append(cnt, np.uint64(3))))
    elif case == "second overflows twice":
        ds[65] = _with_absent(ds[65], np.setdiff1d(_distinct(rng, 1, 1 << 40, 1100), present))
    elif case == "first retries":
        T0 = t0(st, ds[:64])
        w = (1 << 64) // T0
        # T0 grows with the keys added: place them by the T0 that results
        for _ in range(4):
            extra = np.setdiff1d(_distinct(rng, w, w + w // 4, 1100), present)
            d3 = _with_absent(ds[3], extra)
            T1 = t0(st, ds[:3] + [d3] + ds[4:64])
            if T1 == T0:
                break
            T0, w = T1, (1 << 64) // T1
        ds[3] = d3
    else:
        raise KeyError(case)
    return st, ds


def hygiene_inputs():
    """The two flagged calls of test_gpu_kfold_seams.py's hygiene test: one the prep refuses
    (node ids >= 1024 in the state's context), one that overflows bucket 0 at T0 and at 8 T0
    (unhashed keys)."""
    return (random_fold(30, n_keys=2000, k=6, n_nodes=40, node_base=1000),
            random_fold(31, n_keys=3000, k=6, hashed=False))
