"""GPU parity: libdeltagpu (through its C-ABI, on cuda:0) against the C oracle and
the golden fixtures.  Integer work => bit-exact equality everywhere."""
import numpy as np
import pytest
import torch

from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd._abi import CapacityError, FunctionClauseError
from delta_crdt_ex_amd.store import Context, Store, u64
from oracle import ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def up(rep):
    rows, ctx = rep["rows"], rep["ctx"]
    return Store.from_numpy(*rows, device=DEV), Context.from_numpy(ctx[0], ctx[1], ctx[2], DEV)


def rows_eq(got: Store, want):
    g = got.to_numpy()
    assert got.n == len(want[0]), (got.n, len(want[0]))
    for i, (x, y) in enumerate(zip(g, want)):
        assert np.array_equal(x, y), f"column {i} differs"


def ctx_eq(got: Context, want):
    assert got.kind == want[0]
    node, cnt = got.to_numpy()
    assert np.array_equal(node, want[1]) and np.array_equal(cnt, want[2])


def check_join(engine, a, b, keys=None):
    sa, ca = up(a)
    sb, cb = up(b)
    kt = None
    if keys is not None:
        ku = np.unique(np.asarray(keys, np.uint64))
        kt = torch.from_numpy(ku.view(np.int64)).to(DEV)
    out, octx = engine.join2(sa, ca, sb, cb, keys=kt)
    wrows, wctx = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"], keys=keys)
    rows_eq(out, wrows)
    ctx_eq(octx, wctx)
    return out, octx


CASES = [
    dict(n_keys=40, ts_range=1 << 40, dense_ctx=True, ctx_kind=W.VV),
    dict(n_keys=40, ts_range=2, dense_ctx=True, ctx_kind=W.VV),
    dict(n_keys=40, ts_range=1 << 40, dense_ctx=False, ctx_kind=W.VV),
    dict(n_keys=30, ts_range=4, dense_ctx=False, ctx_kind=W.DOTS),
    dict(n_keys=30, ts_range=4, dense_ctx=True, ctx_kind=W.DOTS),
    dict(n_keys=0, ts_range=4, dense_ctx=True, ctx_kind=W.VV),
    dict(n_keys=3000, ts_range=1 << 20, dense_ctx=False, ctx_kind=W.VV),   # multi-tile
    dict(n_keys=2000, ts_range=3, dense_ctx=False, ctx_kind=W.DOTS),       # multi-tile, ties
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("seed", range(4))
def test_join2_random(engine, case, seed):
    rng = np.random.default_rng(1000 * case + seed)
    a, b = W.random_pair(rng, **CASES[case])
    check_join(engine, a, b)
    check_join(engine, b, a)
    keys = np.unique(np.concatenate([a["rows"][0], b["rows"][0]]))
    if len(keys):
        check_join(engine, a, b, keys=keys[::2])
        check_join(engine, a, b, keys=np.concatenate([keys[1::3], np.array([12345], np.uint64)]))


@pytest.mark.parametrize("n_keys", [200_000, 3_000_000])  # fused splits / partition launch
def test_join2_keyed_slices(engine, n_keys):
    """Keyed joins through the per-tile keyset slices: sparse keysets (a few keys per
    tile: the slice staged in LDS), a clustered run of keys (tiles whose slice is longer
    than the LDS slice: global search) next to tiles with no key at all, keys absent
    from both stores, and every key."""
    a, b = W.config2(n_keys=n_keys, seed=21)
    keys = np.unique(np.concatenate([a["rows"][0], b["rows"][0]]))
    rng = np.random.default_rng(n_keys)
    sparse = np.concatenate([rng.choice(keys, len(keys) // 100, replace=False),
                             rng.integers(0, 2**63, 50, dtype=np.uint64)])
    lo = len(keys) // 3
    clustered = np.concatenate([keys[lo:lo + 5000], keys[::997]])
    for ks in (sparse, clustered, keys, np.zeros(0, np.uint64)):
        check_join(engine, a, b, keys=ks)


def test_join2_identical_and_subset(engine):
    """Every row duplicated across the stores: dedup at every tile seam."""
    a, b = W.config2(n_keys=20000, seed=9)
    check_join(engine, a, a)
    # b's store as a subset of a's, contexts equal
    sub = {"rows": tuple(c[::3] for c in a["rows"]), "ctx": a["ctx"]}
    check_join(engine, a, sub)
    check_join(engine, sub, a)


def test_join2_empty_sides(engine):
    a, b = W.config2(n_keys=5000, seed=3)
    empty = {"rows": R.empty_rows(0), "ctx": W.vv({})}
    check_join(engine, a, empty)
    check_join(engine, empty, b)
    check_join(engine, empty, empty)


def test_join2_config2_full_size(engine):
    """BASELINE config 2 at its full size (1M keys, 2M rows in)."""
    a, b = W.config2()
    out, octx = check_join(engine, a, b)
    assert 1_050_000 < out.n < 1_150_000
    engine.store_check(out)


def test_join2_properties_full_size(engine):
    """Size-independent CRDT laws at config-2 size: commutativity, idempotence."""
    a, b = W.config2(seed=11)
    sa, ca = up(a)
    sb, cb = up(b)
    ab, cab = engine.join2(sa, ca, sb, cb)
    ba, cba = engine.join2(sb, cb, sa, ca)
    for x, y in zip(ab.to_numpy(), ba.to_numpy()):
        assert np.array_equal(x, y)
    aa, caa = engine.join2(ab, cab, ab, cab)
    for x, y in zip(aa.to_numpy(), ab.to_numpy()):
        assert np.array_equal(x, y)


def test_join2_capacity_error(engine):
    a, b = W.config2(n_keys=1000, seed=1)
    sa, ca = up(a)
    sb, cb = up(b)
    small = Store.empty(10, DEV)
    with pytest.raises(CapacityError):
        engine.join2(sa, ca, sb, cb, out=small)


def test_join2_async_counts(engine):
    a, b = W.config2(n_keys=50000, seed=4)
    sa, ca = up(a)
    sb, cb = up(b)
    out = Store.empty(sa.n + sb.n, DEV)
    octx = Context.empty(0, ca.n + cb.n, DEV)
    d = torch.zeros(8, dtype=torch.int64, device=DEV)
    for _ in range(3):
        engine.join2_async(sa, ca, sb, cb, out, octx, d_counts=d)
    engine.sync()
    out.n, octx.n = int(d[0]), int(d[1])
    wrows, wctx = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"])
    rows_eq(out, wrows)
    ctx_eq(octx, wctx)


@pytest.mark.parametrize("seed", range(6))
def test_read_lww(engine, seed):
    rng = np.random.default_rng(seed)
    a, _ = W.random_pair(rng, n_keys=3000 if seed % 2 else 50, ts_range=3)
    s, _c = up(a)
    ok, ov = engine.read_lww(s)
    wk, wv = R.read_lww(a["rows"])
    assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)
    sub = wk[::3]
    kt = torch.from_numpy(np.ascontiguousarray(sub).view(np.int64)).to(DEV)
    ok, ov = engine.read_lww(s, keys=kt)
    wk, wv = R.read_lww(a["rows"], keys=sub)
    assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)


def runs_store(rng, lens, ts_range):
    """A sorted, unique store whose key i has lens[i] rows (values ascending, ts drawn
    from a small range so LWW ties are common)."""
    n = int(lens.sum())
    keys = np.sort(rng.choice(2**62, len(lens), replace=False).astype(np.uint64))
    key = np.repeat(keys, lens)
    val = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    ts = rng.integers(-ts_range, ts_range, n).astype(np.int64)
    node = rng.integers(0, 64, n).astype(np.uint32)
    cnt = np.arange(1, n + 1, dtype=np.uint64)
    o = np.lexsort((cnt, node, ts, val, key))
    return tuple(c[o] for c in (key, val, ts, node, cnt))


@pytest.mark.parametrize("shape", ["short", "up_to_32", "long", "giant", "tile_seams"])
def test_read_lww_run_lengths(engine, shape):
    """read/1 over key runs of every length: the segmented reduction carries a run across
    lanes, waves and tiles (1024 rows), with ts ties broken toward the earlier row."""
    rng = np.random.default_rng(len(shape))
    if shape == "short":
        lens = rng.integers(1, 4, 30000)
    elif shape == "up_to_32":
        lens = rng.integers(1, 33, 20000)
    elif shape == "long":
        lens = rng.integers(1, 3000, 300)
    elif shape == "giant":
        lens = np.array([3, 70000, 1, 5000, 2], np.int64)
    else:  # runs ending exactly at, and one row past, tile seams
        lens = np.array([1024, 1023, 2, 1024, 1025, 63, 65, 64, 1, 2048], np.int64)
    rows = runs_store(rng, lens.astype(np.int64), ts_range=3)
    s = Store.from_numpy(*rows, device=DEV)
    ok, ov = engine.read_lww(s)
    wk, wv = R.read_lww(rows)
    assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)
    sub = wk[1::2]
    kt = torch.from_numpy(np.ascontiguousarray(sub).view(np.int64)).to(DEV)
    ok, ov = engine.read_lww(s, keys=kt)
    wk, wv = R.read_lww(rows, keys=sub)
    assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)


# ------------------------------------------------------------------ dg_take_keys, long runs
# take_keys_kernel maps a 256-key tile's output rows to their keys through LDS while the
# tile takes at most 1024 rows (TAKE_TILE, MAPCAP in csrc/take.hip); past that every output
# row binary-searches the tile's offsets.

TAKE_RUNS = np.array([1, 2, 3, 4, 5, 7, 8, 9, 12, 13], np.int64)


def _kt(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(DEV)


def _check_take(engine, rows, s, ks):
    got = engine.take_keys(s, _kt(ks))
    sel = np.isin(rows[0], ks)
    assert got.n == int(sel.sum())
    rows_eq(got, tuple(c[sel] for c in rows))
    return sel


def _tile_rows(rows, ks):
    """Rows each 256-key tile of the key list takes."""
    ukeys, cnt = np.unique(rows[0], return_counts=True)
    pos = np.searchsorted(ukeys, ks)
    hit = ukeys[np.minimum(pos, len(ukeys) - 1)] == ks
    per_key = np.where(hit, cnt[np.minimum(pos, len(ukeys) - 1)], 0)
    return [int(per_key[t:t + 256].sum()) for t in range(0, len(ks), 256)]


def test_take_keys_tiles_past_the_lds_map(engine):
    """600 keys of 1..13 rows: tiles 0 and 1 take about 1,640 rows each (searched offsets),
    tile 2 takes 88 keys' (mapped).  Then with every third key -- and each tile's first and
    last -- replaced by an absent one, so empty ranges share an offset with their
    neighbours; the searching tiles still take more than 1024 rows."""
    rng = np.random.default_rng(17)
    rows = runs_store(rng, TAKE_RUNS[np.arange(600) % 10], ts_range=3)
    s = Store.from_numpy(*rows, device=DEV)
    keys = np.unique(rows[0])
    assert len(keys) == 600
    per_tile = _tile_rows(rows, keys)
    assert per_tile[0] > 1024 and per_tile[1] > 1024 and per_tile[2] <= 1024
    assert _check_take(engine, rows, s, keys).all()
    gone = np.unique(np.concatenate([np.arange(0, 600, 3), [0, 255, 256, 511, 512, 599]]))
    ks = keys.copy()
    ks[gone] = keys[gone] + np.uint64(1)
    assert bool(np.all(ks[1:] > ks[:-1])) and not np.isin(ks[gone], keys).any()
    per_tile = _tile_rows(rows, ks)
    assert per_tile[0] > 1024 and per_tile[1] > 1024 and 0 < per_tile[2] <= 1024
    _check_take(engine, rows, s, ks)


@pytest.mark.parametrize("n_keys,last_run", [(594, 4), (597, 8)])
def test_take_keys_last_run_ends_the_store(engine, n_keys, last_run):
    """The last key's run is exactly 4 / 8 rows and ends at the store's last row: the
    four-rows-a-round walk reaches s.n on a full round (its end clamp)."""
    rng = np.random.default_rng(n_keys)
    lens = TAKE_RUNS[np.arange(n_keys) % 10]
    assert lens[-1] == last_run
    rows = runs_store(rng, lens, ts_range=3)
    s = Store.from_numpy(*rows, device=DEV)
    keys = np.unique(rows[0])
    assert int((rows[0] == keys[-1]).sum()) == last_run and rows[0][-1] == keys[-1]
    assert _check_take(engine, rows, s, keys).all()
    assert int(_check_take(engine, rows, s, keys[-1:]).sum()) == last_run
    _check_take(engine, rows, s, np.array([keys[0], keys[-1], keys[-1] + np.uint64(1)], np.uint64))


def test_read_lww_config2(engine):
    a, b = W.config2()
    rows, _ = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"])
    s = Store.from_numpy(*rows, device=DEV)
    ok, ov = engine.read_lww(s)
    wk, wv = R.read_lww(rows)
    assert np.array_equal(u64(ok), wk) and np.array_equal(u64(ov), wv)


@pytest.mark.parametrize("seed", range(6))
def test_context_union_and_compress(engine, seed):
    rng = np.random.default_rng(seed)
    kinds = [(W.VV, W.VV), (W.DOTS, W.DOTS), (W.VV, W.DOTS)][seed % 3]
    a, _ = W.random_pair(rng, n_keys=200, ctx_kind=kinds[0], dense_ctx=False)
    b, _ = W.random_pair(rng, n_keys=200, ctx_kind=kinds[1], dense_ctx=False)
    _, ca = up(a)
    _, cb = up(b)
    ctx_eq(engine.context_union(ca, cb), R.context_union(a["ctx"], b["ctx"]))
    ctx_eq(engine.context_union(cb, ca), R.context_union(b["ctx"], a["ctx"]))
    if a["ctx"][0] == W.DOTS:
        ctx_eq(engine.compress_dots(ca), R.compress_dots(a["ctx"]))
    else:
        with pytest.raises(FunctionClauseError):
            engine.compress_dots(ca)


def test_large_dot_set_union(engine):
    n = 20000
    rng = np.random.default_rng(5)
    def dots():
        nd = np.sort(rng.integers(0, 50, n).astype(np.uint32))
        c = rng.integers(1, 10**6, n).astype(np.uint64)
        o = np.lexsort((c, nd))
        pairs = np.unique(np.stack([nd[o].astype(np.uint64), c[o]], 1), axis=0)
        return (W.DOTS, pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint64))
    x, y = dots(), dots()
    cx = Context.from_numpy(*x, DEV)
    cy = Context.from_numpy(*y, DEV)
    ctx_eq(engine.context_union(cx, cy), R.context_union(x, y))
    ctx_eq(engine.compress_dots(cx), R.compress_dots(x))


@pytest.mark.parametrize("seed", range(3))
def test_joink(engine, seed):
    rng = np.random.default_rng(50 + seed)
    reps = []
    for _ in range(3):
        a, b = W.random_pair(rng, n_keys=400, ts_range=8, dense_ctx=bool(seed % 2))
        reps += [a, b]
    stores, ctxs = zip(*[up(r) for r in reps])
    out, octx = engine.joink(list(stores), list(ctxs))
    wr, wc = R.joink([r["rows"] for r in reps], [r["ctx"] for r in reps])
    rows_eq(out, wr)
    ctx_eq(octx, wc)


def test_store_check_detects_unsorted(engine):
    a, _ = W.config2(n_keys=3000, seed=2)
    rows = list(a["rows"])
    s = Store.from_numpy(*rows, device=DEV)
    engine.store_check(s)
    rows = [c.copy() for c in rows]
    rows[0][[10, 11]] = rows[0][[11, 10]]
    bad = Store.from_numpy(*rows, device=DEV)
    with pytest.raises(Exception):
        engine.store_check(bad)


# ------------------------------------------------------------------ dg_sort_store (marshalling)

def _np_sorted_unique(rows):
    k, v, t, n, c = (np.asarray(x) for x in rows)
    o = np.lexsort((c, n, t, v, k))
    cols = [x[o] for x in (k, v, t, n, c)]
    if len(cols[0]) > 1:
        keep = np.ones(len(cols[0]), bool)
        keep[1:] = ~np.all([x[1:] == x[:-1] for x in cols], axis=0)
        cols = [x[keep] for x in cols]
    return tuple(cols)


def _shuffled(rows, rng, dup_frac=0.0):
    n = len(rows[0])
    order = rng.permutation(n)
    if dup_frac and n:
        order = np.concatenate([order, rng.choice(n, int(n * dup_frac))])
        order = rng.permutation(order)
    return tuple(np.ascontiguousarray(c[order]) for c in rows)


@pytest.mark.parametrize("n,seed", [(0, 0), (1, 1), (17, 2), (4095, 3), (4097, 4), (70_000, 5)])
def test_sort_store_random(engine, n, seed):
    rng = np.random.default_rng(seed)
    rows = (rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64),
            rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64),
            rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(0, 1 << 64, n, dtype=np.uint64))
    rows = _shuffled(rows, rng, dup_frac=0.1)
    s = Store.from_numpy(*rows, device=DEV)
    s.n = len(rows[0])
    rows_eq(engine.sort_store(s), _np_sorted_unique(rows))


def test_sort_store_ties_everywhere(engine):
    """Equal keys with many entries, equal (key, val) with ts ties of both signs, equal
    (key, val, ts) with several dots: the order falls through every field."""
    rng = np.random.default_rng(9)
    n = 50_000
    rows = (rng.integers(0, 40, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15),
            rng.integers(0, 5, n).astype(np.uint64), rng.integers(-3, 3, n).astype(np.int64),
            rng.integers(0, 4, n).astype(np.uint32), rng.integers(0, 1 << 40, n).astype(np.uint64))
    rows = _shuffled(rows, rng, dup_frac=0.3)
    s = Store.from_numpy(*rows, device=DEV)
    got = engine.sort_store(s)
    rows_eq(got, _np_sorted_unique(rows))
    engine.store_check(got)


def test_sort_then_join_equals_oracle(engine):
    """Config-2 replicas marshalled in a map-walk order (shuffled), sorted on the device,
    then joined: bit-exact with the oracle's join of the sorted replicas."""
    rng = np.random.default_rng(4)
    a, b = W.config2(n_keys=60_000, seed=4)
    sa = engine.sort_store(Store.from_numpy(*_shuffled(a["rows"], rng), device=DEV))
    sb = engine.sort_store(Store.from_numpy(*_shuffled(b["rows"], rng), device=DEV))
    ca = engine.sort_context(Context.from_numpy(a["ctx"][0], *[x[::-1].copy() for x in a["ctx"][1:]], DEV))
    cb = engine.sort_context(Context.from_numpy(b["ctx"][0], *[x[::-1].copy() for x in b["ctx"][1:]], DEV))
    out, octx = engine.join2(sa, ca, sb, cb)
    wr, wc = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"])
    rows_eq(out, wr)
    ctx_eq(octx, wc)


def test_sort_context_dots(engine):
    rng = np.random.default_rng(2)
    n = 30_000
    pairs = np.unique(np.stack([rng.integers(0, 70, n), rng.integers(0, 1 << 50, n)], 1), axis=0)
    perm = rng.permutation(len(pairs))
    c = Context.from_numpy(W.DOTS, pairs[perm, 0].astype(np.uint32), pairs[perm, 1].astype(np.uint64), DEV)
    got = engine.sort_context(c)
    ctx_eq(got, (W.DOTS, pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint64)))


def test_remap_values_region_local(engine):
    """dg_remap_values rewrites only the relabelled region's ids (ids outside
    [old_ids[0], old_ids[-1]] -- canonical integers, the other region -- stay), keeps the
    store sorted, and refuses an id inside the region that its table lacks."""
    from delta_crdt_ex_amd._abi import DeltaGpuError
    key = np.repeat(np.arange(1, 5, dtype=np.uint64), 4)
    val = np.tile(np.array([5, 1 << 60, (1 << 60) + 8, 1 << 63], np.uint64), 4)
    rows = (key, val, np.zeros(16, np.int64), np.zeros(16, np.uint32),
            np.arange(1, 17, dtype=np.uint64))
    s = Store.from_numpy(*rows, device=DEV)
    old = np.array([1 << 60, (1 << 60) + 8], np.uint64)
    new = np.array([(1 << 60) - 100, (1 << 60) + 100], np.uint64)
    engine.remap_values(s, old, new)
    got = s.to_numpy()[1]
    want = val.copy()
    want[val == old[0]], want[val == old[1]] = new[0], new[1]
    assert np.array_equal(got, want)
    engine.store_check(s)
    with pytest.raises(DeltaGpuError):  # rows hold (1 << 60) -+ 100: inside, not in the table
        engine.remap_values(s, np.array([(1 << 60) - 200, (1 << 60) + 200], np.uint64),
                            np.array([(1 << 60) - 300, (1 << 60) + 300], np.uint64))


@pytest.mark.parametrize("n_ids,n_rows", [(2047, 10_000), (2048, 10_000), (2049, 10_000), (5000, 10_000),
                                          (2049, 0), (2049, 1), (2049, 1023), (2049, 1025)])
def test_remap_values_table_sizes(engine, n_ids, n_rows):
    """Id tables at, below and above the 2048 entries remap_values_kernel stages in LDS
    (larger ones are searched in global memory): rows holding table ids (the first and last
    among them), ids below and above the region and canonical integers, against a numpy
    lookup; and an id inside the region that the table lacks is refused."""
    from delta_crdt_ex_amd._abi import DeltaGpuError
    rng = np.random.default_rng(n_ids + n_rows)
    old = np.uint64(1 << 40) + np.cumsum(rng.integers(2, 10, n_ids)).astype(np.uint64)
    new = old[0] + np.arange(n_ids, dtype=np.uint64) * np.uint64(2)  # ascending, inside the region
    assert bool(np.all(old[1:] > old[:-1])) and new[-1] <= old[-1]

    def store_of(val):
        n = len(val)
        key = (np.arange(n) // 50).astype(np.uint64)
        o = np.lexsort((val, key))
        rows = (key, val[o], np.zeros(n, np.int64), np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint64))
        return rows, Store.from_numpy(*rows, device=DEV)

    outside = np.array([0, 5, old[0] - np.uint64(1), old[-1] + np.uint64(1), 1 << 57], np.uint64)
    pool = np.concatenate([old[rng.integers(0, n_ids, 4 * n_rows // 10)], outside[rng.integers(0, 5, 3 * n_rows // 10)],
                           rng.integers(1 << 58, 1 << 63, n_rows, dtype=np.uint64)])[:max(n_rows - 2, 0)]
    val = rng.permutation(np.concatenate([pool, old[[0, -1]]]))[:n_rows]
    rows, s = store_of(val)
    assert s.n == n_rows
    engine.remap_values(s, old, new)
    v = rows[1]
    j = np.minimum(np.searchsorted(old, v), n_ids - 1)
    want = np.where(old[j] == v, new[j], v)
    if n_rows >= 1000:
        assert (want != v).sum() > n_rows // 4 and (want == v).sum() > n_rows // 4
    assert np.array_equal(s.to_numpy()[1], want)
    engine.store_check(s)
    if n_ids == 5000 and n_rows:
        stale = old[n_ids // 2] + np.uint64(1)  # (the gaps are at least 2)
        assert stale not in old
        bad = val.copy()
        bad[n_rows // 3] = stale
        _, sb = store_of(bad)
        with pytest.raises(DeltaGpuError):
            engine.remap_values(sb, old, new)


# ------------------------------------------------------------------ dg_sort_store, large and degenerate
# digit_scan_kernel scans a digit's tile counts 256 tiles a round and carries between the
# rounds (more than 1,048,576 rows); sort_scan_kernel likewise past 1024 tiles (4,194,304 rows).

@pytest.mark.parametrize("n,dups", [(4096, 0), (4096, 1000), (8192, 0), (8192, 1000), (1_048_576, 0),
                                    (1_048_576, 1000), (1_048_577, 1000), (4_194_305, 1000)])
def test_sort_store_large(engine, n, dups):
    """Rows in order by construction (ascending keys, val = the row's rank; ts of both
    signs, node and cnt random, so every byte pass runs), shuffled, with `dups` rows
    repeated at the end: n an exact multiple of the 4096-row tile, one past 256 tiles, one
    past 1024 tiles."""
    rng = np.random.default_rng(n + dups)
    want = (np.sort(rng.integers(0, 1 << 64, n, dtype=np.uint64)), np.arange(n, dtype=np.uint64),
            rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64),
            rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(0, 1 << 64, n, dtype=np.uint64))
    order = np.concatenate([rng.permutation(n), rng.integers(0, n, dups)])
    s = Store.from_numpy(*(c[order] for c in want), device=DEV)
    assert s.n == n + dups
    got = engine.sort_store(s)
    rows_eq(got, want)
    engine.store_check(got)


@pytest.mark.parametrize("case", ["only key varies", "only ts varies", "only cnt's low byte, in order",
                                  "identical rows"])
def test_sort_store_skipped_passes(engine, case):
    """Fields whose every byte is constant: all of their passes are skipped, and the
    identity order (no index array yet) is carried into the next field."""
    rng = np.random.default_rng(len(case))
    n = 5000
    key, val = np.full(n, 0x1234567890ABCDEF, np.uint64), np.full(n, 1 << 62, np.uint64)
    ts, node, cnt = np.full(n, -5, np.int64), np.full(n, 3, np.uint32), np.full(n, 77, np.uint64)
    if case == "only key varies":
        key = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    elif case == "only ts varies":
        ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
        assert (ts < 0).any() and (ts > 0).any()
    elif case == "only cnt's low byte, in order":
        cnt = np.sort(rng.integers(0, 256, n)).astype(np.uint64)
    rows = (key, val, ts, node, cnt)
    want = _np_sorted_unique(rows)
    assert len(want[0]) == {"only key varies": n, "only ts varies": n, "only cnt's low byte, in order": 256,
                            "identical rows": 1}[case]
    got = engine.sort_store(Store.from_numpy(*rows, device=DEV))
    rows_eq(got, want)
    engine.store_check(got)


def test_sort_context_vv_and_large_dot_list(engine):
    """dg_sort_context of a VV (3,000 distinct nodes, reversed: one field) and of a dot list
    of 1,048,577 distinct pairs (one past 256 tiles), shuffled."""
    nodes = np.arange(3000, dtype=np.uint32) * np.uint32(7) + np.uint32(1)
    cnts = np.arange(3000, dtype=np.uint64) ** 2 + np.uint64(1)
    got = engine.sort_context(Context.from_numpy(W.VV, nodes[::-1].copy(), cnts[::-1].copy(), DEV))
    ctx_eq(got, (W.VV, nodes, cnts))
    rng = np.random.default_rng(8)
    n = 1_048_577
    node = rng.integers(0, 70, n).astype(np.uint32)
    cnt = np.arange(n, dtype=np.uint64) * np.uint64(1 << 20) + rng.integers(0, 1 << 20, n).astype(np.uint64)
    perm = rng.permutation(n)
    node, cnt = node[perm], cnt[perm]
    got = engine.sort_context(Context.from_numpy(W.DOTS, node, cnt, DEV))
    o = np.lexsort((cnt, node))
    ctx_eq(got, (W.DOTS, node[o], cnt[o]))
