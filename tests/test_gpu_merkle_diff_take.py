"""dg_merkle_diff_take (csrc/merkle_diff.hip, the take form): the full Merkle diff answered with
the kept keys' rows of one of the two stores, in one call.

Checker: keys and total against the C oracle's store_diff; rows against a numpy mask of the chosen
store's rows over the kept keys (the oracle's rows, not the library's); offs against
np.searchsorted on those rows' keys; and equality with Engine.merkle_diff + Engine.take_keys,
which the take form leaves untouched.  Both sides run in every case.  The cases and the path each
subtree takes (LDS stage / global merge) are diff_take_cases.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import diff_take_cases as D
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd._abi import DeltaGpuError
from delta_crdt_ex_amd.store import Store, u64
from oracle import ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COLS = ("key", "val", "ts", "node", "cnt")

_built = {}  # (case name, depth) -> stores, trees and the oracle's diff: built once, never modified


def built(engine, name, depth=None, shard_bits=0, shard=0):
    case = D.by_name(name)
    depth = case.depth if depth is None else depth
    key = (name, depth, shard_bits, shard)
    if key not in _built:
        rows = D.pair(case)
        if shard_bits:
            rows = tuple(tuple(c[(r[0] >> np.uint64(64 - shard_bits)) == shard] for c in r) for r in rows)
        stores = tuple(Store.from_numpy(*r, device=DEV) for r in rows)
        trees = tuple(engine.merkle_build(s, depth, shard_bits=shard_bits, shard=shard) for s in stores)
        _built[key] = (rows, stores, trees, R.store_diff(*rows))
    return _built[key]


def expected(rows, keys):
    """the chosen store's rows over `keys` and the keys' row offsets, by numpy"""
    m = np.isin(rows[0], keys)
    exp = tuple(np.asarray(c)[m] for c in rows)
    offs = np.searchsorted(exp[0], np.append(keys, np.uint64(2**64 - 1)), side="left").astype(np.uint64)
    offs[-1] = len(exp[0])
    return exp, offs


def check(engine, b, side, cap=None):
    rows, stores, trees, want = b
    kept = want if cap is None else want[:cap]
    keys, got, offs, total = engine.merkle_diff_take(trees[0], trees[1], side=side, cap=cap)
    assert total == len(want)
    assert np.array_equal(u64(keys), kept)
    exp, eoffs = expected(rows[side], kept)
    assert got.n == len(exp[0])
    for name, g, e in zip(COLS, got.to_numpy(), exp):
        assert np.array_equal(g, e), name
    o = offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(o, eoffs)
    assert int(o[len(kept)]) == got.n
    # the two calls it replaces
    k2 = engine.merkle_diff(trees[0], trees[1], cap=cap)
    assert torch.equal(keys, k2)
    t2 = engine.take_keys(stores[side], k2)
    assert t2.n == got.n
    for g, e in zip(got.to_numpy(), t2.to_numpy()):
        assert np.array_equal(g, e)
    return len(kept), got.n


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_rows_of_the_differing_keys(engine, name, side):
    nk, nr = check(engine, built(engine, name), side)
    assert nk > 0
    if name.startswith("hot") and len(D.pair(D.by_name(name))[side][0]) == 599:
        assert nr >= 200  # the 200-row run is among the rows of the store that holds it


@pytest.mark.parametrize("name", ["random3000_d14", "merkle20000_d21"])
def test_truncation_keeps_a_prefix(engine, name):
    """cap cuts inside exactly one subtree; the subtrees before it are whole, so the row prefix is
    exact: rows and offs are the prefix's, offs[n_out] == rows.n."""
    b = built(engine, name)
    want, depth = b[3], D.by_name(name).depth
    first = int(np.sum((want >> np.uint64(64 - depth + 12)) == (want[0] >> np.uint64(64 - depth + 12))))
    assert 1 <= first < len(want)
    for cap in sorted({0, 1, max(first // 2, 1), first, len(want) - 1, len(want), len(want) + 1000}):
        for side in (0, 1):
            nk, _ = check(engine, b, side, cap)
            assert nk == min(cap, len(want))


def raw_call(engine, trees, stores, side, cap, out, offs, rows):
    n, tot = C.c_uint64(), C.c_uint64()
    ta, tb, sa, sb = trees[0].abi(), trees[1].abi(), stores[0].abi(), stores[1].abi()
    so = rows.abi() if isinstance(rows, Store) else rows
    rc = engine.lib.dg_merkle_diff_take(engine.h, C.byref(ta), C.byref(sa), C.byref(tb), C.byref(sb), side,
                                        C.cast(out.data_ptr(), _abi.P64) if isinstance(out, torch.Tensor) else out,
                                        cap,
                                        C.cast(offs.data_ptr(), _abi.P64) if isinstance(offs, torch.Tensor) else offs,
                                        C.byref(so), C.byref(n), C.byref(tot))
    return rc, int(n.value), int(tot.value), so


def test_row_capacity(engine):
    """one row too few: DG_E_CAPACITY, rows.n the number needed, the keys valid; exactly enough: fine"""
    rows, stores, trees, want = b = built(engine, "random300_d12")
    for side in (0, 1):
        exp, eoffs = expected(rows[side], want)
        need = len(exp[0])
        out = torch.zeros(len(want), dtype=torch.int64, device=DEV)
        offs = torch.zeros(len(want) + 1, dtype=torch.int64, device=DEV)
        small = Store.empty(need - 1, DEV)
        assert small.cap == need - 1
        rc, n, tot, so = raw_call(engine, trees, stores, side, len(want), out, offs, small)
        assert rc == _abi.DG_E_CAPACITY
        assert (n, tot, int(so.n)) == (len(want), len(want), need)
        assert np.array_equal(u64(out), want)
        exact = Store.empty(need, DEV)
        rc, n, tot, so = raw_call(engine, trees, stores, side, len(want), out, offs, exact)
        assert rc == _abi.DG_OK and int(so.n) == need
        exact._set(so)
        for g, e in zip(exact.to_numpy(), exp):
            assert np.array_equal(g, e)
        assert np.array_equal(offs.cpu().numpy().view(np.uint64), eoffs)
    # the binding sizes the rows itself and retries with the size the call asked for
    keys, got, offs, total = engine.merkle_diff_take(trees[0], trees[1], side=1, rows=Store.empty(3, DEV))
    assert got.n == len(expected(rows[1], want)[0][0]) and total == len(want)


def test_an_empty_store_each_way_and_equal_stores(engine):
    rows = D.pair(D.by_name("random300_d12"))[0]
    full = Store.from_numpy(*rows, device=DEV)
    none = Store.from_numpy(*R.empty_rows(), device=DEV)
    none.n = 0
    tf, tn = engine.merkle_build(full, 12), engine.merkle_build(none, 12)
    allkeys = np.unique(rows[0])
    for (ta, tb), full_side in (((tf, tn), 0), ((tn, tf), 1)):
        for side in (0, 1):
            keys, got, offs, total = engine.merkle_diff_take(ta, tb, side=side)
            assert total == len(allkeys) and np.array_equal(u64(keys), allkeys)
            o = offs.cpu().numpy().view(np.uint64)
            if side == full_side:
                assert got.n == len(rows[0])
                for g, e in zip(got.to_numpy(), rows):
                    assert np.array_equal(g, e)
                assert np.array_equal(o, expected(rows, allkeys)[1])
            else:
                assert got.n == 0 and not o.any()
    for side in (0, 1):
        keys, got, offs, total = engine.merkle_diff_take(tf, tf, side=side)
        assert (keys.numel(), got.n, total) == (0, 0, 0)
        assert offs.cpu().numpy().tolist() == [0]


def test_outputs_in_page_locked_host_memory(engine):
    rows, stores, trees, want = built(engine, "random300_d12")
    exp, eoffs = expected(rows[1], want)
    nk, nr = len(want), len(exp[0])
    sizes = [8 * nk, 8 * (nk + 1), 8 * nr, 8 * nr, 8 * nr, 4 * nr + 4, 8 * nr]
    p = C.c_void_p()
    _abi.check(engine.lib.dg_host_alloc(engine.h, sum(sizes), C.byref(p)))
    try:
        at = [p.value + sum(sizes[:i]) for i in range(len(sizes))]
        so = _abi.dg_store(at[2], at[3], at[4], at[5], at[6], 0, nr)
        rc, n, tot, so = raw_call(engine, trees, stores, 1, nk, C.cast(at[0], _abi.P64), C.cast(at[1], _abi.P64), so)
        assert (rc, n, tot, int(so.n)) == (_abi.DG_OK, nk, nk, nr)
        view = lambda a, dt, m: np.frombuffer((C.c_char * (np.dtype(dt).itemsize * m)).from_address(a), dt).copy()
        assert np.array_equal(view(at[0], np.uint64, nk), want)
        assert np.array_equal(view(at[1], np.uint64, nk + 1), eoffs)
        for a, e in zip(at[2:], exp):
            assert np.array_equal(view(a, e.dtype, nr), e)
    finally:
        engine.lib.dg_host_free(engine.h, p)


def test_a_shard_tree_pair_over_the_shards_store(engine):
    for shard in (0, 1):
        b = built(engine, "random3000_d12", depth=11, shard_bits=1, shard=shard)
        assert len(b[3]) > 0
        for side in (0, 1):
            check(engine, b, side)
            check(engine, b, side, cap=len(b[3]) // 2)


def test_a_store_the_tree_does_not_describe_leaves_the_outputs_untouched(engine):
    """A store cut short under its tree (as test_diff_against_a_store_the_index_does_not_describe
    makes one): DG_E_INVAL, no row read past the store, and nothing written -- also by the subtrees
    before the one that overruns, which alone would pass their own check."""
    rng = np.random.default_rng(23)
    a, b = W.random_pair(rng, 50_000, n_nodes=4, max_entries=3)
    sa, sb = Store.from_numpy(*a["rows"], device=DEV), Store.from_numpy(*b["rows"], device=DEV)
    ta, tb = engine.merkle_build(sa, 14), engine.merkle_build(sb, 14)
    cap = 1000
    for cut in (a["rows"][0].size // 2, 10):
        short = Store.from_numpy(*(c[:cut] for c in a["rows"]), device=DEV)
        for starts in (ta.starts, None):
            kept, ta.starts = ta.starts, starts
            try:
                for side in (0, 1):
                    out = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
                    offs = torch.full((cap + 1,), -7, dtype=torch.int64, device=DEV)
                    got = Store.empty(4 * cap, DEV)
                    for c in COLS:
                        getattr(got, c).fill_(-7)
                    rc, n, tot, so = raw_call(engine, (ta, tb), (short, sb), side, cap, out, offs, got)
                    assert rc == _abi.DG_E_INVAL and b"more rows than its store" in engine.lib.dg_last_error()
                    assert (n, tot, int(so.n)) == (0, 0, 0)
                    for t in (out, offs, *(getattr(got, c) for c in COLS)):
                        assert bool((t == -7).all())
            finally:
                ta.starts = kept
    # the engine is usable after the error
    keys, got, offs, total = engine.merkle_diff_take(ta, tb, side=0, cap=cap)
    want = R.store_diff(a["rows"], b["rows"])
    assert total == len(want) and np.array_equal(u64(keys), want[:cap])


def test_interleaved_with_the_plain_diff_at_two_depths(engine):
    """The group sums -- keys and rows -- are zeroed by the next call's write kernel, by parity;
    a take between two diffs of another depth (512 subtrees in two groups, then 4) and the
    reverse leave every call correct."""
    deep, flat = built(engine, "merkle20000_d21"), built(engine, "merkle20000_d14")
    for first, second in ((deep, flat), (flat, deep)):
        for _ in range(2):
            assert np.array_equal(u64(engine.merkle_diff(*first[2])), first[3])
            check(engine, second, 1)
            assert np.array_equal(u64(engine.merkle_diff(*first[2])), first[3])
            check(engine, first, 0)
            check(engine, second, 0)


def test_bad_side_is_rejected(engine):
    rows, stores, trees, want = built(engine, "random300_d12")
    with pytest.raises(DeltaGpuError):
        engine.merkle_diff_take(trees[0], trees[1], side=2)
