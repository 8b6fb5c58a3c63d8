"""Crafted calls for dg_join_delta's in-place write (csrc/dg_kdw.h, after kdelta.hip's count
kernel): a state of 3,000 hashed keys with 1 to 8 rows each under a VV context, and one
sync-shaped delta whose 600-key keyset -- three count tiles of KD_BLOCK = 256, the last one
partial -- keeps EVERY key's row count, while keys of several rows lose rows and gain as many.
Written in place in tuple order, such a key's output slot overtakes the state row still to be
read: naive_in_place restates that loop and bites() lists the keys it gets wrong, so
tests/test_inplace_cases.py can prove with the C oracle alone that a GPU pass on a case
means the kernel avoided the read-back.  Test data only (seeded numpy).

The dots decide each row's fate (aw_lww_map.ex:196-209), over four nodes from node_base up:
  S  kept rows: the delta's context does not name the node
  Z  removed rows: the delta's context covers them and the delta holds none of them
  K  kept rows the delta holds too (its context covers them: the `same row` branch)
  D  inserted rows: counters above the state's VV entry for D
Keys outside the keyset carry S, Z and K dots that the delta's context covers as well: the
keyed join must leave them alone."""
import functools

import numpy as np

from keyed_fold_cases import rows_from

VV, DOTS = 0, 1
V0 = 1 << 62
KD_BLOCK, KD_RUN, KVT = 256, 64, 1024
N_KEYS, N_KEYSET, N_RANDOM = 3000, 600, 150
SEED = 11
D_FLOOR = 5  # the state's VV entry for node D (no state row carries a D dot)

# name -> (keyset position, state rows, removed positions, gaps of the inserted rows (gap g is
# before state row g), positions of kept rows the delta holds too)
NAMED = {
    "front": (0, 3, (2,), (0,), ()),           # [X, Y, Z] -> [D, X, Y]
    "middle": (255, 4, (3,), (1,), ()),        # [X, Y, W, Z] -> [X, D, Y, W]
    "two": (256, 4, (2, 3), (0, 0), ()),       # [X, Y, Z1, Z2] -> [D1, D2, X, Y]
    "wide": (599, KD_RUN, (KD_RUN - 1,), (0,), ()),
    "back": (100, 3, (0,), (3,), ()),          # [Z, X, Y] -> [X, Y, D']
    "pair": (300, 2, (1,), (0,), ()),          # [X, Z] -> [D, X]
    "shared": (400, 3, (2,), (3,), (0,)),      # [X, Y, Z] -> [X, Y, D'], X in the delta too
    "one": (550, 1, (0,), (0,), ()),           # [Z] -> [D]
}
BITING = ("front", "middle", "two", "wide")
HARMLESS = ("back", "pair", "shared", "one")


def key_rows(rows, x):
    """the rows of key x as tuples, in store order"""
    lo, hi = np.searchsorted(rows[0], np.uint64(x), "left"), np.searchsorted(rows[0], np.uint64(x), "right")
    return [tuple(int(c[i]) for c in rows) for i in range(lo, hi)]


def ctx_of(kind, dots):
    """the context covering `dots` [(node, cnt)]: a VV of the per-node maxima, or the dots"""
    if kind == VV:
        top = {}
        for n, c in dots:
            top[n] = max(top.get(n, 0), c)
        nodes = sorted(top)
        return (VV, np.array(nodes, np.uint32), np.array([top[n] for n in nodes], np.uint64))
    d = sorted(set(dots))
    return (DOTS, np.array([n for n, _ in d], np.uint32), np.array([c for _, c in d], np.uint64))


@functools.lru_cache(maxsize=None)
def case(delta_ctx=VV, node_base=0, variant="hazard", seed=SEED):
    """variant: `hazard` the count-preserving call; `quiet` the same state, only the one-row key
    `one` changes; `one_moves` hazard plus one key the state lacks; `outside` hazard plus a
    one-row key in the upper half of the key space (outside shard 0 of 2), replaced by one row.
    Returns state, delta, keys, named {name: key}, random / filler key lists, per-key delta
    rows and dots (alone()), extra (the added key or None).  Shared between tests: read only."""
    assert variant in ("hazard", "quiet", "one_moves", "outside")
    rng = np.random.default_rng(seed)
    S, Z, K, D = (node_base + i for i in range(4))
    keys = np.unique(rng.integers(0, 1 << 63, N_KEYS + 50, dtype=np.uint64))[:N_KEYS]
    assert len(keys) == N_KEYS
    keyset = keys[np.sort(rng.choice(N_KEYS, N_KEYSET, replace=False))]
    in_set = set(keyset.tolist())
    named = {name: int(keyset[spec[0]]) for name, spec in NAMED.items()}
    free = np.setdiff1d(np.arange(N_KEYSET), [s[0] for s in NAMED.values()])
    rpos = set(rng.choice(free, N_RANDOM, replace=False).tolist())
    random_keys = [int(keyset[p]) for p in sorted(rpos)]
    filler = [int(keyset[p]) for p in free if p not in rpos]
    nxt = {S: 0, Z: 0, K: 0, D: D_FLOOR}

    def dot(node):
        nxt[node] += 1
        return (node, nxt[node])

    state, drows, ddots = [], {}, {}

    def emit(x, na, removed, gaps, shared):
        dr, dd = drows.setdefault(x, []), ddots.setdefault(x, [])
        for i in range(na):
            node = Z if i in removed else K if i in shared else S
            r = (x, V0 + 16 * (i + 1), int(rng.integers(0, 8))) + dot(node)
            state.append(r)
            if node == K:
                dr.append(r)
            if node != S:
                dd.append(r[3:])
        for j, g in enumerate(gaps):
            r = (x, V0 + 16 * g + 1 + j, int(rng.integers(0, 8))) + dot(D)
            dr.append(r)
            dd.append(r[3:])

    # `one` and the filler first, so that a VV over their dots alone covers no dot of the
    # other keyset keys (quiet); then the keys outside the keyset; then the keys that bite
    emit(named["one"], *NAMED["one"][1:])
    for x in filler:
        na = int(rng.integers(1, 9))
        emit(x, na, (), (), tuple(i for i in range(na) if rng.random() < 0.1))
    quiet_keys = [named["one"]] + filler
    for x in keys.tolist():
        if x in in_set:
            continue
        for i in range(int(rng.integers(1, 9))):
            state.append((x, V0 + 16 * (i + 1), int(rng.integers(0, 8))) + dot((S, Z, K)[int(rng.integers(0, 3))]))
    for name, spec in NAMED.items():
        if name != "one":
            emit(named[name], *spec[1:])
    for x in random_keys:
        na = int(rng.integers(2, 13))
        r = min(int(rng.integers(1, 4)), na)
        removed = set(rng.choice(na, r, replace=False).tolist())
        gaps = sorted(rng.integers(0, na + 1, r).tolist())
        emit(x, na, removed, gaps, tuple(i for i in range(na) if i not in removed and rng.random() < 0.25))
    extra = None
    if variant == "one_moves":
        extra = int(keyset[300]) + 1
        assert extra not in set(keys.tolist())
        emit(extra, 0, (), (0,), ())
    elif variant == "outside":
        extra = (1 << 63) + 99
        emit(extra, 1, (0,), (0,), ())
    call = quiet_keys if variant == "quiet" else list(drows)
    ks = keyset if extra is None else np.union1d(keyset, np.array([extra], np.uint64))
    top = {}
    for r in state:
        top[r[3]] = max(top.get(r[3], 0), r[4])
    top[D] = D_FLOOR
    return {"state": {"rows": rows_from(state), "ctx": ctx_of(VV, list(top.items()))},
            "delta": {"rows": rows_from([r for x in call for r in drows[x]]),
                      "ctx": ctx_of(delta_ctx, [d for x in call for d in ddots[x]])},
            "keys": ks, "named": named, "random": random_keys, "filler": filler, "extra": extra,
            "delta_ctx": delta_ctx, "drows": drows, "ddots": ddots,
            "params": (delta_ctx, node_base, variant, seed)}


def alone(c, name):
    """key `name` of case c as a call of its own: (delta, keys) -- its delta rows, a context
    over its dots, a one-key keyset"""
    x = c["named"][name]
    return ({"rows": rows_from(c["drows"][x]), "ctx": ctx_of(c["delta_ctx"], c["ddots"][x])},
            np.array([x], np.uint64))


def naive_in_place(state_rows, joined_rows, key):
    """dg_kdw.h's write loop over a plain list: the key's kept state rows and its new rows
    merged in tuple order into the state's own slots -- store slot o, THEN load the next kept
    state row from the list that is being overwritten.  Returns the slots afterwards."""
    buf = key_rows(state_rows, key)
    want = key_rows(joined_rows, key)
    keep = [r in want for r in buf]                  # amask
    new = [r for r in want if r not in buf]          # the delta rows that come in (dmask)
    na, nd = len(buf), len(new)
    i = j = o = 0
    while i < na and not keep[i]:
        i += 1
    ra = buf[i] if i < na else None
    rb = new[j] if j < nd else None
    while i < na or j < nd:
        take_a = j >= nd or (i < na and ra < rb)
        r = ra if take_a else rb
        if o < na:
            buf[o] = r
        else:
            buf.append(r)
        o += 1
        if take_a:
            i += 1
            while i < na and not keep[i]:
                i += 1
            if i < na:
                ra = buf[i]
        else:
            j += 1
            if j < nd:
                rb = new[j]
    return buf[:o]


def reads_back(state_rows, joined_rows, key):
    """kdelta.hip's rule for sending a call through the spare store, restated: walking the
    key's rows in tuple order, the write has stored `wo` rows -- every kept and every new row so
    far -- when it loads kept state row i; wo > i means slot i holds an output row by then."""
    old, want = key_rows(state_rows, key), key_rows(joined_rows, key)
    wo, out = 0, 0
    for r in sorted(set(old) | set(want)):
        if r in want:
            if r in old and wo > old.index(r):
                return True
            out += 1
            if r in old:
                wo = out
    return False


@functools.lru_cache(maxsize=None)
def _joined(delta_ctx, node_base, variant, seed):
    from oracle import ref as R
    c = case(delta_ctx, node_base, variant, seed)
    return R.join2(c["state"]["rows"], c["state"]["ctx"], c["delta"]["rows"], c["delta"]["ctx"], keys=c["keys"])


def joined(c):
    """the oracle's keyed join of case c, computed once: (rows, context)"""
    return _joined(*c["params"])


def bites(c):
    """the keyset keys whose rows naive_in_place gets wrong (against the oracle's join)"""
    want = joined(c)[0]
    return [int(x) for x in c["keys"] if naive_in_place(c["state"]["rows"], want, x) != key_rows(want, x)]
