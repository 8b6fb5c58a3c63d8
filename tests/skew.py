"""Key sets that are NOT uniform hashes, and CPU models of the two device searches whose
fallbacks only such key sets reach (helper module: no tests).

Every workload generator draws key ids as 64-bit hashes, and the device searches are tuned
for that: interp_lower_bound (csrc/dg_device.h) brackets a uniform key in its six
interpolation rounds, mp_split (csrc/dg_jsplit.h) in its first 64-wide window.  The key sets
here send them to their exact fallbacks (the plain binary search, mp_search's 128-ary
search); the models count which exit a lookup takes, so tests/test_skew_models.py can
assert that the inputs of tests/test_gpu_skewed_keys.py do reach those exits."""
import functools
import math

import numpy as np

from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.interning import splitmix64_np
from oracle import ref as R

TOP = (1 << 64) - 1


# ---------------------------------------------------------------- key-set generators
# Each: a sorted unique uint64 array of exactly n keys from the seeded rng (over-draw, cut).

def _cut(draw, n):
    """At least n distinct draws (the callers cut them to n)."""
    m = n + n // 4 + 16
    while True:
        u = np.unique(draw(m))
        if len(u) >= n:
            return u
        m *= 2


def uniform(rng, n):
    """The control: uniform over the whole key space, like hashed ids."""
    u = _cut(lambda m: rng.integers(0, 1 << 64, m, dtype=np.uint64), n)
    return np.sort(rng.choice(u, n, replace=False))


def geometric(rng, n):
    """2^U[0, 63.9): as many keys below 2^32 as above it."""
    u = _cut(lambda m: (2.0 ** rng.uniform(0, 63.9, m)).astype(np.uint64), n)
    return np.sort(rng.choice(u, n, replace=False))


def two_clusters(rng, n):
    """Half of the keys in [0, 2^24), half in [2^64 - 2^24, 2^64), with 0 and 2^64 - 1."""
    assert n >= 2
    nl = n // 2
    nh = n - nl
    low = _cut(lambda m: rng.integers(1, 1 << 24, m, dtype=np.uint64), nl - 1)
    low = rng.choice(low, nl - 1, replace=False)
    high = _cut(lambda m: rng.integers(1, 1 << 24, m, dtype=np.uint64), nh - 1)
    high = np.uint64(TOP) - rng.choice(high, nh - 1, replace=False)
    return np.sort(np.concatenate([np.array([0], np.uint64), low, high, np.array([TOP], np.uint64)]))


def dense_plus_max(rng, n):
    """3 i for i < n - 1, and 2^64 - 1 (rng unused: the set is fixed by n)."""
    return np.concatenate([np.arange(n - 1, dtype=np.uint64) * np.uint64(3), np.array([TOP], np.uint64)])


GENERATORS = {"uniform": uniform, "geometric": geometric, "two_clusters": two_clusters,
              "dense_plus_max": dense_plus_max}
SKEWED = ("geometric", "two_clusters", "dense_plus_max")


# ---------------------------------------------------------------- rekeyed replicas

def union_keys(reps):
    return np.unique(np.concatenate([r["rows"][0] for r in reps] + [np.zeros(0, np.uint64)]))


def rekey(reps, keyset):
    """The replicas with the i-th smallest key id of their rows' union replaced by keyset[i],
    and the map itself (for keysets handed to calls).  The map is strictly increasing, so
    the stores stay sorted and unique, and the oracle's result on the rekeyed replicas is
    the same map of its result on the originals."""
    old = union_keys(reps)
    keyset = np.asarray(keyset, np.uint64)
    assert len(keyset) == len(old) and (len(old) < 2 or bool(np.all(keyset[1:] > keyset[:-1])))

    def remap(keys):
        keys = np.asarray(keys, np.uint64)
        i = np.searchsorted(old, keys)
        assert np.array_equal(old[np.minimum(i, len(old) - 1)], keys), "a key outside the replicas' union"
        return keyset[i]

    out = [{**r, "rows": (remap(r["rows"][0]),) + tuple(r["rows"][1:])} for r in reps]
    return out, remap


# The base replicas of tests/test_gpu_skewed_keys.py: about 15 join tiles, the smallest
# shape that still has several mp_split boundaries and lookups that outlast six rounds.
BASE_KEYS, BIG_KEYS = 5_000, 20_000
# (dense_plus_max: a seed with which BOTH replicas hold the largest key -- random_pair drops
# 30 % of the keys per replica, and without 2^64 - 1 a replica's keys are just 3 i, which
# interpolation finds at once)
SEED = {"uniform": 101, "geometric": 102, "two_clusters": 103, "dense_plus_max": 114}


@functools.lru_cache(maxsize=None)
def _random_pair(seed, n_keys):
    return W.random_pair(np.random.default_rng(seed), n_keys, n_nodes=5, ts_range=1 << 10)


@functools.lru_cache(maxsize=None)
def skewed_pair(name, n_keys=BASE_KEYS):
    """W.random_pair(rng, n_keys, n_nodes=5, ts_range=1 << 10) with both replicas rekeyed to
    one key set of the named generator."""
    a, b = _random_pair(SEED[name], n_keys)
    ks = GENERATORS[name](np.random.default_rng(SEED[name] + 1000), len(union_keys([a, b])))
    (a, b), _ = rekey([a, b], ks)
    return a, b


@functools.lru_cache(maxsize=None)
def disjoint_pair(name, n_keys=BASE_KEYS):
    """A: a random_pair replica rekeyed to the named generator's key set.  B: a replica of
    an independent random_pair on uniform keys, none of them in A."""
    a, _ = _random_pair(SEED[name], n_keys)
    _, b = _random_pair(SEED[name] + 500, n_keys)
    (a,), _ = rekey([a], GENERATORS[name](np.random.default_rng(SEED[name] + 1000), len(union_keys([a]))))
    nb = len(union_keys([b]))
    u = uniform(np.random.default_rng(SEED[name] + 2000), nb + 64)
    u = u[~np.isin(u, a["rows"][0])][:nb]
    (b,), _ = rekey([b], u)
    return a, b


def take_lists(key_col):
    """The key lists the take / read tests look up in a store with this key column."""
    u = np.unique(key_col)
    absent = np.setdiff1d(u[u != np.uint64(TOP)] + np.uint64(1), u)
    return {"every key": u, "every 7th": u[::7], "key + 1 (absent)": absent,
            "first and last five": np.unique(np.concatenate([u[:5], u[-5:]]))}


HOT_KEYS, HOT_RUN, HOT_SEED = 5_000, 20_000, 105


def hot_key_state(rng, n_keys, run):
    """Hashed keys, one row per key, except the key a third of the way in, which holds `run`
    rows: distinct (val, ts), distinct dots on nodes 0..3, and a VV covering every dot.
    Returns (replica, hot key)."""
    keys = np.unique(splitmix64_np(rng.choice(1 << 40, n_keys + 16, replace=False).astype(np.uint64)))[:n_keys]
    assert len(keys) == n_keys
    hot = keys[n_keys // 3]
    key = np.sort(np.concatenate([keys, np.full(run - 1, hot, np.uint64)]))
    n = len(key)
    val = np.uint64(1 << 62) + rng.permutation(n).astype(np.uint64)
    ts = rng.permutation(n).astype(np.int64) - n // 2
    j = rng.permutation(n)
    node = (j % 4).astype(np.uint32)
    cnt = (j // 4 + 1).astype(np.uint64)
    rows = W.sort_rows(key, val, ts, node, cnt)
    ctx = (R.VV, np.arange(4, dtype=np.uint32), np.full(4, (n + 3) // 4, np.uint64))
    return {"rows": rows, "ctx": ctx}, hot


@functools.lru_cache(maxsize=None)
def hot_state():
    return hot_key_state(np.random.default_rng(HOT_SEED), HOT_KEYS, HOT_RUN)


# ---------------------------------------------------------------- models

def model_interp_lower_bound(k, x):
    """interp_lower_bound(k, 0, len(k), x) of csrc/dg_device.h, line by line.  k: ascending
    keys (a list of ints, or an array).  Returns (index, path): `early` (decided by the
    store's first and last key), `window` (the bracket fell to <= 16 rows within the six
    rounds) or `binary` (the round budget spent: the plain binary search)."""
    if isinstance(k, np.ndarray):
        k = k.tolist()
    x = int(x)
    lo, hi = 0, len(k)
    if lo >= hi:
        return lo, "early"
    kl, kh = k[lo], k[hi - 1]
    if x <= kl:
        return lo, "early"
    if x > kh:
        return hi, "early"
    a, b = lo, hi - 1  # k[a] < x <= k[b]
    it = 0
    while it < 6 and b - a > 16:
        m = float(b - a)
        f = float(x - kl) / float(kh - kl)
        g = float(a) + f * m
        e = 2.0 * math.sqrt(m * f * (1.0 - f)) + 4.0
        lo_g, hi_g = g - e, g + e
        g0 = a + 1 if lo_g <= float(a + 1) else (b - 1 if lo_g >= float(b - 1) else int(lo_g))
        g1 = a + 1 if hi_g <= float(a + 1) else (b - 1 if hi_g >= float(b - 1) else int(hi_g))
        k0, k1 = k[g0], k[g1]
        if k0 >= x:
            b, kh = g0, k0
        elif k1 < x:
            a, kl = g1, k1
        else:
            a, kl, b, kh = g0, k0, g1, k1
        it += 1
    if b - a <= 16:
        c = 0
        for j in range(1, 16):
            v = k[a + j if a + j < b else a]
            c += 1 if (a + j < b and v < x) else 0
        return a + 1 + c, "window"
    l2, h2 = a + 1, b
    while l2 < h2:
        mid = (l2 + h2) >> 1
        if k[mid] < x:
            l2 = mid + 1
        else:
            h2 = mid
    return l2, "binary"


WAVE, PK = 64, 128


def _mp_pred(A, B, d, i):
    # mp_pred of csrc/dg_jsplit.h for disjoint key sets: the keys never tie, so no full row is read
    return A[i] < B[d - 1 - i]


def _model_mp_search(A, B, d, lo, hi):
    """mp_search of csrc/dg_jsplit.h: first i in [lo, hi) with NOT mp_pred(i), 128-ary."""
    for _ in range(64):
        if not hi > lo:
            break
        span = hi - lo
        if span <= PK:
            xs = [lo + s for s in range(PK)]
            fs = [x < hi and not _mp_pred(A, B, d, x) for x in xs]
        else:
            xs = [lo + (span * (s + 1)) // (PK + 1) for s in range(PK)]
            fs = [not _mp_pred(A, B, d, x) for x in xs]
        kf = fs.index(True) if True in fs else PK  # first false sample
        if span <= PK:
            return lo + kf if kf < span else hi
        if kf == PK:
            lo = lo + (span * PK) // (PK + 1) + 1
        else:
            nh = lo + (span * (kf + 1)) // (PK + 1)
            if kf > 0:
                lo = lo + (span * kf) // (PK + 1) + 1
            hi = nh
    return lo


def model_mp_split(A_keys, B_keys, d):
    """mp_split of csrc/dg_jsplit.h, line by line, for two stores whose key sets are disjoint
    (only keys are compared).  A_keys, B_keys: the stores' key columns.  Returns
    (split, path): `short` (a diagonal of at most 128 candidates: mp_search at once),
    `win0` / `win1` / `win2` (bracketed by that 64-wide window) or `search` (three windows
    without a bracket: the 128-ary mp_search over the whole diagonal)."""
    A = A_keys.tolist() if isinstance(A_keys, np.ndarray) else A_keys
    B = B_keys.tolist() if isinstance(B_keys, np.ndarray) else B_keys
    na, nb = len(A), len(B)
    total = na + nb
    lo, hi = (d - nb if d > nb else 0), min(d, na)
    if hi - lo <= PK:
        return _model_mp_search(A, B, d, lo, hi), "short"
    scale = float(na) * float(nb) / (float(total) * 18446744073709551616.0)
    lim = float(hi - lo)

    def shifted(c):
        gap = float(B[d - 1 - c]) - float(A[c])
        sft = gap * scale
        sft = lim if sft > lim else (-lim if sft < -lim else sft)
        ni = c + int(sft)
        return lo if ni < lo else (hi - 1 if ni > hi - 1 else ni)

    i = int(float(d) * float(na) / float(total))
    i = min(max(i, lo), hi - 1)
    i = shifted(i)
    for r in range(3):
        wlo = i - WAVE // 2 if i > lo + WAVE // 2 else lo
        whi = min(wlo + WAVE, hi)
        wlo = whi - WAVE if whi - WAVE > lo else lo  # (whi >= lo + 64: the diagonal is longer than 128)
        kf = whi - wlo
        for lane in range(WAVE):
            x0 = wlo + lane
            if x0 < whi and not _mp_pred(A, B, d, x0):
                kf = lane
                break
        if (kf > 0 or wlo == lo) and (kf < whi - wlo or whi == hi):
            return wlo + kf, "win%d" % r
        i = shifted((wlo + whi) // 2)
    return _model_mp_search(A, B, d, lo, hi), "search"


def true_split(A_keys, B_keys, d):
    """#A rows among the first d rows of the merge of two stores with disjoint key sets."""
    both = np.concatenate([A_keys, B_keys])
    from_a = np.argsort(both, kind="stable") < len(A_keys)
    return int(from_a[:d].sum())


JT = 1016  # merged positions per join tile (csrc/dg_launch.h JOIN_TILE)


def boundaries(na, nb, jt=JT):
    """The interior tile boundaries' diagonals of a join of na + nb rows."""
    return list(range(jt, na + nb, jt))


def interp_paths(k, queries):
    k = k.tolist() if isinstance(k, np.ndarray) else k
    return [model_interp_lower_bound(k, int(x))[1] for x in np.asarray(queries, np.uint64)]


def split_paths(A_keys, B_keys):
    A, B = A_keys.tolist(), B_keys.tolist()
    return [model_mp_split(A, B, d)[1] for d in boundaries(len(A), len(B))]
