"""dg_mark_ids on the device, and the interning sweeps built on it.

The mark pass answers "which ids of this table occur in this column of these stores"; the
expected flags come from numpy.isin.  The implementation's paths and their boundaries
(csrc/mark.hip), each with a size on either side here:

  * table size 2048 | 2049: the whole table staged in LDS (MARK_STAGED) | not;
  * value column above 2048 ids (MARK_SAMPLED): every stride-th id staged, stride =
    ceil(n_ids / 2048): 4096 (stride 2) | 4097 (stride 3);
  * key column above 2048 ids (MARK_WINDOW): a tile's window of the table, 2048 ids (staged
    in LDS, with its marks) | 2049 ids (searched and marked in global memory);
  * tile size: 2048 rows; on the key column 512 rows while all stores together make at most
    4096 such tiles: 4096 * 512 = 2,097,152 rows | one more;
  * rows per store 512 | 513 (key column) and 2048 | 2049: one tile | two; 256 | 257 rows:
    the 16-byte loads of the workgroup's first 128 threads | a third wave's; odd row counts
    end in a lone 8-byte row;
  * a column whose address is not 16-byte aligned takes 8-byte loads.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.store import Context, Store

pytestmark = pytest.mark.gpu

KEY, VAL = _abi.DG_COL_KEY, _abi.DG_COL_VAL
CANON_LO, CANON_HI = 1 << 58, 1 << 63


def table(rng, n, column):
    """n strictly ascending ids: any u64 for keys; outside the canonical range for values"""
    if n == 0:
        return np.zeros(0, np.uint64)
    out = np.zeros(0, np.uint64)
    while len(out) < n:
        x = rng.integers(1, 1 << 63, size=2 * n + 16, dtype=np.uint64)
        if column == VAL:  # the low region (0, 2^58) and the high region [2^63, 2^64)
            low = rng.random(len(x)) < 0.25
            x = np.where(low, x >> np.uint64(6), x | np.uint64(1 << 63))
            x = x[(x > 0) & ((x < CANON_LO) | (x >= CANON_HI))]
        else:
            x = x * np.uint64(2) + np.uint64(1)
        out = np.unique(np.concatenate([out, x]))
    return np.sort(rng.choice(out, size=n, replace=False))


def column(rng, n, ids, column_, p_known=0.7, p_canon=0.15, pool=None):
    """n ids for a store's column: table ids (a random subset `pool` of them, so that some
    table ids stay unused), canonical integers (value column), ids the table lacks"""
    c = rng.integers(1, 1 << 62, size=n, dtype=np.uint64) * np.uint64(2)  # even: not in a key table
    if column_ == VAL:
        c = c | np.uint64(1 << 63)
        c = c[~np.isin(c, ids)] if len(ids) else c
        c = np.resize(c, n) if len(c) else np.full(n, (1 << 63) + 5, np.uint64)
    r = rng.random(n)
    if len(ids):
        pool = ids if pool is None else pool
        known = r < p_known
        c[known] = rng.choice(pool, size=int(known.sum()))
    if column_ == VAL:
        canon = r > 1 - p_canon
        c[canon] = rng.integers(CANON_LO, CANON_HI, size=int(canon.sum()), dtype=np.uint64)
    return c


def make_store(rng, n, ids, col, dev, **kw):
    """a store of n rows, sorted by key as every store is"""
    if n == 0:
        return Store.empty(1, dev), np.zeros(0, np.uint64)
    if col == KEY:
        key = np.sort(column(rng, n, ids, KEY, **kw))  # repeats: several rows of a key
        val = rng.integers(CANON_LO, CANON_HI, size=n, dtype=np.uint64)
        marked = key
    else:
        key = np.sort(rng.integers(0, 1 << 63, size=n, dtype=np.uint64))
        val = column(rng, n, ids, VAL, **kw)
        # a key's rows often share a value: runs of equal ids exercise the skipped searches
        run = rng.random(n) < 0.3
        run[0] = False
        idx = np.arange(n)
        idx[run] = 0
        val = val[np.maximum.accumulate(idx)]
        marked = val
    st = Store.from_numpy(key, val, np.arange(n, dtype=np.int64), np.zeros(n, np.uint32),
                          np.arange(1, n + 1, dtype=np.uint64), dev)
    return st, marked


def expect(cols, ids, col):
    rows = np.concatenate(cols) if cols else np.zeros(0, np.uint64)
    used = np.isin(ids, rows).astype(np.uint8)
    missing = ~np.isin(rows, ids)
    if col == VAL:
        missing &= ~((rows >= np.uint64(CANON_LO)) & (rows < np.uint64(CANON_HI)))
    return used, int(missing.sum())


def check(engine, stores, cols, ids, col):
    used, n_used, n_unknown = engine.mark_ids(stores, col, ids)
    want, want_unknown = expect(cols, ids, col)
    got = used.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert n_used == int(want.sum())
    assert n_unknown == want_unknown
    return got


@pytest.mark.parametrize("col", [KEY, VAL])
@pytest.mark.parametrize("n_ids", [0, 1, 2047, 2048, 2049, 4096, 4097])
def test_table_sizes(engine, col, n_ids):
    rng = np.random.default_rng(n_ids * 2 + col)
    ids = table(rng, n_ids, col)
    pool = ids[rng.random(n_ids) < 0.6] if n_ids > 1 else ids
    stores, cols = zip(*[make_store(rng, n, ids, col, engine.device, pool=pool if len(pool) else None)
                         for n in (257, 0, 5000)])  # three stores, an empty one in the middle
    got = check(engine, list(stores), list(cols), ids, col)
    if n_ids > 1:
        assert 0 < got.sum() < n_ids  # the case has used and unused ids


@pytest.mark.parametrize("col", [KEY, VAL])
@pytest.mark.parametrize("rows", [[], [0], [1], [255], [256], [257], [511], [512], [513], [2048], [2049],
                                  [100_003], [1, 0, 255], [257, 0, 0, 2049]])
def test_row_counts_and_store_counts(engine, col, rows):
    rng = np.random.default_rng(len(rows) * 1000 + sum(rows) + col)
    for n_ids in (300, 3000):  # the LDS-staged table, and the sampled / windowed search
        ids = table(rng, n_ids, col)
        pool = ids[::3]
        made = [make_store(rng, n, ids, col, engine.device, pool=pool) for n in rows]
        check(engine, [m[0] for m in made], [m[1] for m in made], ids, col)


@pytest.mark.parametrize("col", [KEY, VAL])
@pytest.mark.parametrize("n_ids", [700, 5000])
def test_every_id_used_no_id_used_and_one_row_at_the_very_end(engine, col, n_ids):
    rng = np.random.default_rng(n_ids + col)
    dev = engine.device
    ids = table(rng, n_ids, col)

    def store_of(marked):
        n = len(marked)
        other = rng.integers(CANON_LO, CANON_HI, size=n, dtype=np.uint64)
        if col == KEY:
            marked = np.sort(marked)
            return Store.from_numpy(marked, other, np.arange(n), np.zeros(n), np.arange(n) + 1, dev), marked
        return Store.from_numpy(np.sort(other), marked, np.arange(n), np.zeros(n), np.arange(n) + 1, dev), marked

    # every id used: twice over, spread over two stores (duplicates across stores)
    a, ca = store_of(rng.permutation(np.concatenate([ids, ids[: n_ids // 2]])))
    b, cb = store_of(rng.permutation(ids))
    got = check(engine, [a, b], [ca, cb], ids, col)
    assert got.all()
    # no id used: rows of ids the table lacks (all unknown)
    absent = ids + np.uint64(2)
    absent = absent[~np.isin(absent, ids)]
    c, cc = store_of(absent)
    got = check(engine, [c], [cc], ids, col)
    assert not got.any()
    # one id used, by a single row at the very end of the last store
    if col == KEY:
        lone = np.concatenate([absent[absent < ids[-1]], ids[-1:]])  # the greatest key: the last row
    else:
        lone = np.concatenate([absent, ids[n_ids // 2: n_ids // 2 + 1]])
    d, cd = store_of(lone) if col == KEY else (
        Store.from_numpy(np.arange(len(lone), dtype=np.uint64), lone, np.arange(len(lone)), np.zeros(len(lone)),
                         np.arange(len(lone)) + 1, dev), lone)
    got = check(engine, [c, Store.empty(1, dev), d], [cc, np.zeros(0, np.uint64), cd], ids, col)
    assert got.sum() == 1


def test_every_value_canonical(engine):
    rng = np.random.default_rng(5)
    for n_ids in (100, 3000):
        ids = table(rng, n_ids, VAL)
        n = 3001
        val = rng.integers(CANON_LO, CANON_HI, size=n, dtype=np.uint64)
        st = Store.from_numpy(np.arange(n, dtype=np.uint64), val, np.arange(n), np.zeros(n), np.arange(n) + 1,
                              engine.device)
        used, n_used, n_unknown = engine.mark_ids([st], VAL, ids)
        assert n_used == 0 and n_unknown == 0 and not used.cpu().numpy().any()
        # the same ids in the KEY column are plain unknown keys: canonical values are skipped
        # on the value column only
        keyed = Store.from_numpy(np.sort(val), val, np.arange(n), np.zeros(n), np.arange(n) + 1, engine.device)
        _u, n_used, n_unknown = engine.mark_ids([keyed], KEY, table(rng, n_ids, KEY))
        assert n_used == 0 and n_unknown == n


def test_unknown_counts_rows_not_distinct_ids(engine):
    ids = np.array([10, 20, 30], np.uint64) + np.uint64(1 << 63)
    lost = np.uint64((1 << 63) + 25)
    val = np.array([ids[0]] * 3 + [lost] * 7 + [np.uint64(CANON_LO + 9)] * 5 + [ids[2]], np.uint64)
    n = len(val)
    st = Store.from_numpy(np.arange(n, dtype=np.uint64), val, np.arange(n), np.zeros(n), np.arange(n) + 1,
                          engine.device)
    used, n_used, n_unknown = engine.mark_ids([st, st], VAL, ids)
    assert used.cpu().numpy().tolist() == [1, 0, 1] and n_used == 2
    assert n_unknown == 14  # 7 rows of ONE lost id, in each of the two stores; canonical rows not counted


@pytest.mark.parametrize("window", [2048, 2049])
def test_key_window_boundary(engine, window):
    """One tile whose first and last keys span exactly `window` table ids: 2048 are staged
    in LDS, 2049 are searched in global memory.  Then the same keys in a store large enough
    for 2048-row tiles."""
    rng = np.random.default_rng(window)
    ids = table(rng, 6000, KEY)
    lo = 1500
    span = ids[lo: lo + window]
    inside = rng.choice(span[1:-1], size=300)
    odd_out = span[5:155] + np.uint64(1)  # even keys between table ids: unknown
    odd_out = odd_out[~np.isin(odd_out, ids)]
    key = np.sort(np.concatenate([span[:1], inside, odd_out, span[-1:]]))
    assert len(key) <= 512  # one tile
    n = len(key)
    st = Store.from_numpy(key, np.full(n, CANON_LO, np.uint64), np.arange(n), np.zeros(n), np.arange(n) + 1,
                          engine.device)
    got = check(engine, [st], [key], ids, KEY)
    assert got[lo] and got[lo + window - 1] and not got[:lo].any() and not got[lo + window:].any()


@pytest.mark.parametrize("col", [KEY, VAL])
@pytest.mark.parametrize("rows", [4096 * 512, 4096 * 512 + 1])
def test_tile_size_boundary(engine, col, rows):
    """Key column: 4096 tiles of 512 rows | one row more, 2048-row tiles.  (The value column
    has 2048-row tiles at both sizes; it runs here as the large-store case.)"""
    rng = np.random.default_rng(rows + col)
    ids = table(rng, 20_000, col)
    # two stores, so that the second one's tiles start in the middle of the tile sequence
    made = [make_store(rng, n, ids, col, engine.device, pool=ids[::2], p_known=0.9)
            for n in (rows - 100 * 512, 100 * 512)]  # 3996 (or 3997) + 100 tiles of 512 rows
    check(engine, [m[0] for m in made], [m[1] for m in made], ids, col)


@pytest.mark.parametrize("col", [KEY, VAL])
def test_unaligned_column_and_caller_tensor_ids(engine, col):
    """A column that starts 8 bytes off a 16-byte boundary (a view into a larger buffer), and
    the table passed as a device tensor."""
    rng = np.random.default_rng(77 + col)
    ids = table(rng, 2500, col)
    st, marked = make_store(rng, 4099, ids, col, engine.device, pool=ids[::2])
    shifted = Store(*[torch.cat([c[:1], c])[1:] for c in (st.key, st.val, st.ts, st.node, st.cnt)], st.n)
    assert (shifted.key.data_ptr() % 16, shifted.val.data_ptr() % 16) == (8, 8)
    dev_ids = torch.from_numpy(ids.view(np.int64)).to(engine.device)
    check(engine, [shifted, st], [marked, marked], dev_ids.cpu().numpy().view(np.uint64), col)
    used, _n, _x = engine.mark_ids([shifted], col, dev_ids)
    assert np.array_equal(used.cpu().numpy(), expect([marked], ids, col)[0])


@pytest.mark.parametrize("col", [KEY, VAL])
@pytest.mark.parametrize("n_ids", [5, 3000])
def test_unordered_table_is_refused(engine, col, n_ids):
    rng = np.random.default_rng(n_ids + 3 * col)
    ids = table(rng, n_ids, col)
    st, marked = make_store(rng, 3000, ids, col, engine.device)
    for kind in ("swap", "repeat"):
        bad = ids.copy()
        j = n_ids // 2
        if kind == "swap":
            bad[j], bad[j + 1] = ids[j + 1], ids[j]
        else:
            bad[j + 1] = bad[j]
        with pytest.raises(_abi.DeltaGpuError) as e:
            engine.mark_ids([st], col, bad)
        assert e.value.code == _abi.DG_E_ORDER
    check(engine, [st], [marked], ids, col)  # the engine is fine afterwards


def test_flags_in_host_memory_are_the_same_bytes(engine):
    rng = np.random.default_rng(9)
    lib = engine.lib
    for col, n_ids in ((VAL, 2047), (KEY, 4101)):  # (4101: the unaligned tail of the flag bytes too)
        ids = table(rng, n_ids, col)
        st, marked = make_store(rng, 5000, ids, col, engine.device, pool=ids[::2])
        want = check(engine, [st], [marked], ids, col)
        p = C.c_void_p()
        _abi.check(lib.dg_host_alloc(engine.h, n_ids, C.byref(p)))
        try:
            C.memset(p, 0xEE, n_ids)
            dev_ids = torch.from_numpy(ids.view(np.int64)).to(engine.device)
            torch.cuda.synchronize()
            arr = (_abi.dg_store * 1)(st.abi())
            nu, nx = C.c_uint64(), C.c_uint64()
            _abi.check(lib.dg_mark_ids(engine.h, arr, 1, col, C.cast(C.c_void_p(dev_ids.data_ptr()), _abi.P64),
                                       n_ids, p, C.byref(nu), C.byref(nx)))
            got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n_ids,)).copy()
        finally:
            _abi.check(lib.dg_host_free(engine.h, p))
        assert np.array_equal(got, want) and nu.value == want.sum()


def test_call_right_after_an_async_join_sees_the_joined_rows(engine):
    from delta_crdt_ex_amd import workloads as W
    a, b = W.config2(n_keys=3000, seed=3)
    dev = engine.device
    sa, sb = Store.from_numpy(*a["rows"], device=dev), Store.from_numpy(*b["rows"], device=dev)
    ca, cb = Context.from_numpy(*a["ctx"], dev), Context.from_numpy(*b["ctx"], dev)
    ref, _ = engine.join2(sa, ca, sb, cb)
    k, v, _t, _n, _c = ref.to_numpy()
    out = Store.empty(sa.n + sb.n, dev)
    out.key.zero_()
    out.val.zero_()
    octx = Context.empty(_abi.DG_CTX_VV, ca.n + cb.n, dev)
    ids = np.unique(np.concatenate([a["rows"][0], b["rows"][0]]))  # every key of either side
    engine.join2_async(sa, ca, sb, cb, out, octx)
    out.n = ref.n  # the asynchronous form leaves the count on the device
    used, n_used, n_unknown = engine.mark_ids([out], KEY, ids)
    assert np.array_equal(used.cpu().numpy(), np.isin(ids, k).astype(np.uint8))
    assert n_unknown == 0 and 0 < n_used == len(np.unique(k))


# ---------------------------------------------------------------- through aw_lww_map
@pytest.fixture(scope="module")
def M(engine):
    from delta_crdt_ex_amd import aw_lww_map
    aw_lww_map._ENGINE = engine
    return aw_lww_map


def _value(i, r):
    """the value key i gets in round r: a term of another class each time"""
    from delta_crdt_ex_amd.interning import CANON_LO as INT_LO
    from oracle.erlterm import Atom
    return [f"v{r}-{i}", i + r * 0.5 + 0.25, Atom(f"a{r}_{i}"), (r, f"t{i}"), INT_LO - 1 - (r * 1000 + i),
            r * 1000 + i][(i + r) % 6]


def _reads(d):
    return {repr(k): repr(v) for k, v in d.items()}


def test_end_to_end_sweep_through_aw_lww_map(M):
    from delta_crdt_ex_amd.interning import Universe, is_canonical_int
    from delta_crdt_ex_amd.terms import order_key
    from oracle import awlww_term as T
    U = Universe()
    NK, ROUNDS, NODE = 600, 5, 1
    keys = [f"k{i}" for i in range(NK)]
    # 600 keys, the first values as one marshalled state
    value = {k: {(_value(i, 0), i): frozenset([(NODE, i + 1)])} for i, k in enumerate(keys)}
    ms, ts = M.from_terms(value, {NODE: NK}, U), T.AW({NODE: NK}, value)
    for r in range(1, ROUNDS + 1):  # every key overwritten 5 times, each a join of an add delta
        for i, k in enumerate(keys):
            v, t = _value(i, r), r * 1000 + i
            ms = M.join(ms, M.add(k, v, NODE, ms, ts=t), [k])
            ts = T.join(ts, T.add(k, v, NODE, ts, t), [k])
    for k in keys[::6]:  # 100 keys removed
        ms = M.join(ms, M.remove(k, NODE, ms), [k])
        ts = T.join(ts, T.remove(k, NODE, ts), [k])
    assert ms.rows.n == NK - 100
    assert _reads(M.read(ms)) == _reads(T.read(ts))
    live_values = {order_key(v) for ents in ts.value.values() for (v, _t) in ents if not is_canonical_int(v)}
    assert U.value_count() > 4 * len(live_values) and U.key_count() == NK  # the tables only grew
    tree = M.merkle_map(ms, 8)
    nodes, counts = tree.nodes.cpu().numpy().copy(), tree.bucket_counts().copy()
    epoch, version = U.val_epoch, U.terms_version

    out = M.sweep(U, keys=True)

    assert out["values"][1] == U.value_count() == len(live_values)
    assert {order_key(t) for t in U.value_ids()[1]} == live_values
    assert out["keys"] == (NK, NK - 100) and U.key_count() == NK - 100
    assert U.val_epoch == epoch and U.terms_version != version
    assert _reads(M.read(ms)) == _reads(T.read(ts))
    assert ms.value == ts.value
    after = M.merkle_map(ms, 8)
    assert np.array_equal(after.nodes.cpu().numpy(), nodes) and np.array_equal(after.bucket_counts(), counts)
    assert M.sweep(U, keys=True) == {"values": (len(live_values),) * 2, "keys": (NK - 100,) * 2}

    # one more join: an update of the tree built before the sweep still equals a rebuild
    nxt = M.join(ms, M.add("k1", ("fresh", 1.5), NODE, ms, ts=10 ** 9), ["k1"])
    nxt_t = T.join(ts, T.add("k1", ("fresh", 1.5), NODE, ts, 10 ** 9), ["k1"])
    changed = M.engine().join2_changes(ms.rows, ms.ctx, nxt.rows, nxt.ctx)[2]
    M.engine().merkle_update(tree, nxt.rows, changed)
    fresh = M.merkle_map(nxt, 8)
    assert np.array_equal(tree.nodes.cpu().numpy(), fresh.nodes.cpu().numpy())
    assert np.array_equal(tree.bucket_counts(), fresh.bucket_counts())

    # values interned after the sweep that tie on ts with a survivor: read in term order.
    # k2's and k3's survivors; a concurrent writer (an add from an empty base: nothing removed)
    # adds a dropped term and a new one at the same ts, one below and one above in term order
    empty_m, empty_t = M.compress_dots(M.new(U)), T.compress_dots(T.new())
    for k, w in (("k2", _value(2, 1)), ("k3", "zzzz-after-the-sweep"), ("k4", -1.0e300), ("k5", _value(5, 2))):
        i = int(k[1:])
        t = ROUNDS * 1000 + i  # the survivor's ts
        nxt = M.join(nxt, M.add(k, w, 100 + i, empty_m, ts=t), [k])  # (a writer of its own: a fresh dot)
        nxt_t = T.join(nxt_t, T.add(k, w, 100 + i, empty_t, t), [k])
        assert len(nxt_t.value[k]) == 2  # both entries live: a tie at the greatest ts
    assert _reads(M.read(nxt)) == _reads(T.read(nxt_t))
    assert nxt.value == nxt_t.value
    ids, terms = U.value_ids()
    assert all(a < b for a, b in zip(ids, ids[1:]))
    assert all(order_key(a) < order_key(b) for a, b in zip(terms, terms[1:]))


# ---------------------------------------------------------------- through the NIF mirror
def test_sweep_through_the_nif_mirror():
    from delta_crdt_ex_amd import nif
    from oracle import awlww_term as T
    _ok, eng = nif.engine_open(0)
    try:
        A, B = T.compress_dots(T.new()), T.compress_dots(T.new())
        for i in range(40):
            A = T.join(A, T.add(f"k{i}", f"a{i}", 11, A, 100 + i), [f"k{i}"])
        for i in range(20, 60):
            v = "only-B" if i == 33 else (i + 0.5 if i % 2 else ("b", i))
            B = T.join(B, T.add(f"k{i}", v, 22, B, 200 + i), [f"k{i}"])
        _ok, sa, va = nif.state_load(eng, A.dots, A.value)
        _ok, sb, vb = nif.state_load(eng, B.dots, B.value)
        U = eng.universe
        nobody, only_b = U.value("held by neither"), U.value("only-B")
        gone_key = U.key("a key no state holds")
        n_vals = len({repr(v) for s in (A, B) for ents in s.value.values() for (v, _t) in ents})
        assert U.value_count() == n_vals + 1 and U.key_count() == 61

        assert nif.sweep(eng) == ("ok", {"values": (n_vals + 1, n_vals), "keys": (61, 60)})
        assert U.value_term(only_b) == "only-B"  # held by the second state only
        with pytest.raises(KeyError):
            U.value_term(nobody)
        with pytest.raises(KeyError):
            U.key_term(gone_key)
        assert (sa.version, sb.version) == (va, vb)  # versions unchanged

        assert nif.merkle_build(sa, va, 6) == "ok" and nif.merkle_build(sb, vb, 6) == "ok"
        keys = sorted(set(A.value) | set(B.value))
        r = nif.join_delta(sa, va, B.dots, B.value, keys)
        assert r[0] == "ok", r
        J = T.join(A, B, keys)
        va2 = r[1]
        assert r[2] == J.dots == {11: 40, 22: 40}
        assert _reads(nif.read(sa, va2, "all")[1]) == _reads(T.read(J))
        assert _reads(nif.read(sb, vb, "all")[1]) == _reads(T.read(B))
        assert nif.take(sa, va2, keys)[1] == J.value
        # anti-entropy between the two states: the keys whose value maps differ
        cont = nif.merkle_prepare(sa, va2, 2)[1]
        side = [(sb, vb), (sa, va2)]
        for hop in range(16):
            res = nif.merkle_continue(*side[hop % 2], cont, 2, "infinite")
            if res[0] == "ok":
                break
            cont = res[1]
        assert res[0] == "ok"
        assert sorted(res[1]) == sorted(k for k in keys if J.value.get(k) != B.value.get(k))

        n_now = U.value_count()
        assert nif.sweep(eng) == ("ok", {"values": (n_now, n_now), "keys": (60, 60)})  # nothing left to drop
    finally:
        eng.close()
