"""dg_merkle_continues_take on cuda:0 (csrc/merkle_cont.hip cont_hop_kernel<true, true>): the
batch hop whose leaf-form hops also return the rows of the keys they keep.  X is one side of
tests/partial_diff_cases.py's ladder; the hops are those of tests/cont_batch_cases.py.  Keys are
the C oracle's (cont_batch_cases.answer), rows the numpy selection np.isin(rows_x.key,
keys[:max_sync]) of X's sorted rows, and both are compared with what the existing calls give:
merkle_continues for every element, take_keys for the rows."""
import random

import numpy as np
import pytest
import torch

import cont_batch_cases as B
import partial_diff_cases as P
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.store import u64
from test_gpu_merkle_continues import assert_is, assert_same, dev, dev_cont
from test_gpu_partial_diff import side

pytestmark = pytest.mark.gpu

BR = 16  # rows of a bucket the hop kernel keeps in registers (merkle_cont.hip)


def x_hops(x, max_sync, shard_bits=0, shard=0):
    """(rows_x, hops): X = the ladder's side A against (B, the empty replica, A), or its side B
    against A"""
    a, b, _ = P.ladder(8, shard_bits, shard)
    if x == "a":
        return a, B.ladder_hops(max_sync, 3, shard_bits, shard)
    return b, tuple(B.hops_of(b, (a,), 8, 3, max_sync, shard_bits, shard))


def kept_of(want, max_sync):
    """the keys a keys hop keeps: truncate(keys, max_sync_size)"""
    return want[1] if max_sync is None else want[1][:max_sync]


def expect_rows(rows_x, kept):
    """(columns, offs): Map.take(value, kept) of X's sorted rows and its per-key partition"""
    sel = np.isin(rows_x[0], kept)
    cols = tuple(c[sel] for c in rows_x)
    offs = np.concatenate([np.searchsorted(cols[0], kept, "left"), [len(cols[0])]]).astype(np.uint64)
    return cols, offs


def assert_rows(engine, tree, rows_x, res, kept):
    """a keys hop's element: keys, total aside, the offsets and the rows, column for column,
    against numpy and against take_keys of the kept keys"""
    assert len(res) == 5 and np.array_equal(u64(res[1]), kept)
    cols, offs = expect_rows(rows_x, kept)
    assert np.array_equal(u64(res[3]), offs)
    got = res[4].to_numpy()
    assert res[4].n == len(cols[0]) == int(offs[-1])
    for g, c in zip(got, cols):
        assert g.dtype == c.dtype and np.array_equal(g, c)
    if len(kept):
        for g, c in zip(got, engine.take_keys(tree.store, dev(kept)).to_numpy()):
            assert np.array_equal(g, c)


def check_take(engine, tree, rows_x, hops, max_sync, want, depth=8, **kw):
    """one batch through merkle_continues_take, every element against merkle_continues' and the
    oracle; returns the elements"""
    conts = [dev_cont(rc, depth) for rc, _ in hops]
    plain = engine.merkle_continues(tree, conts, 3, max_sync)
    got = engine.merkle_continues_take(tree, conts, want, 3, max_sync, **kw)
    assert len(got) == len(hops)
    for (rc, w), res, pl, wj in zip(hops, got, plain, want):
        if B.kind_of(w) == "keys" and wj:
            assert pl[0] == "ok" and res[0] == "ok" and res[2] == pl[2] == len(w[1])
            kept = kept_of(w, max_sync)
            assert np.array_equal(u64(pl[1])[: len(kept)], kept)
            assert_rows(engine, tree, rows_x, res, kept)
        else:
            assert len(res) == len(pl)  # no rows: merkle_continues' element
            assert_same(res, pl)
            assert_is(res, w, depth)
    return got


def row_paths(rows_x, hops, max_sync):
    """Which of the kernel's row paths these hops reach, from the oracle's data alone: a cut by
    max_sync inside a bucket of more than 16 rows (the global-memory path) / of at most 16 (the
    register path); a key of more than 16 rows; a key X lacks; a hop with no rows at all."""
    tx = B.tree_of(rows_x, 8)
    reached = set()
    for _, w in hops:
        if B.kind_of(w) != "keys":
            continue
        kept = kept_of(w, max_sync)
        if len(kept) < len(w[1]):
            last, nxt = tx.bucket_of(w[1][len(kept) - 1: len(kept) + 1])
            if last == nxt and tx.counts[last] > BR:
                reached.add("cut_big")
            if last == nxt and 0 < tx.counts[last] <= BR:
                reached.add("cut_small")
        per_key = [int(np.count_nonzero(rows_x[0] == k)) for k in kept]
        reached |= {name for name, on in (("long_key", max(per_key) > BR), ("absent", min(per_key) == 0),
                                          ("no_rows", sum(per_key) == 0)) if on}
    return reached


CASES = [(x, ms) for x in ("a", "b") for ms in (None, 200, 5, 1)]


@pytest.mark.parametrize("x,max_sync", CASES)
def test_parity_with_the_two_calls(engine, x, max_sync):
    """Before a case trusts itself: the hops of CASES -- the very hops these cases run -- reach
    every row path between them, by the oracle's data."""
    reached = set().union(*(row_paths(x_hops(cx, cm)[0], x_hops(cx, cm)[1], cm) for cx, cm in CASES))
    assert reached == {"cut_big", "cut_small", "long_key", "absent", "no_rows"}
    rows_x, hops = x_hops(x, max_sync)
    kinds = {B.kind_of(w) for _, w in hops}
    assert "keys" in kinds and "node" in kinds
    got = check_take(engine, side(engine, rows_x, 8)[0], rows_x, hops, max_sync, [True] * len(hops))
    assert any(len(r) == 5 for r in got)


def test_mixed_batch(engine):
    """Node-form hops, a leaf-out hop, keys hops with and without a take, an empty input and a
    position outside the tree: hops without a take are merkle_continues' exactly, no rows where
    the answer is not keys, and the bad hop leaves the others' rows intact."""
    rows_x, hops = x_hops("a", None)
    assert {B.kind_of(w) for _, w in hops} == {"node", "leaf", "keys", "empty"}
    tree = side(engine, rows_x, 8)[0]
    conts = [dev_cont(rc, 8) for rc, _ in hops]
    node = next(j for j, (rc, _) in enumerate(hops) if rc[0] == "node")
    bad = dev_cont(B.bad_position(hops[node][0]), 8)
    empty = dev_cont(B.empty_input(3), 8)
    order = conts[:2] + [bad] + conts[2:] + [empty]
    keys_hops = [j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "keys"]
    assert len(keys_hops) >= 2
    want = [j not in keys_hops[1::2] for j in range(len(hops))]  # every other keys hop without a take
    wants = want[:2] + [True] + want[2:] + [True]
    caps = [(4096, 512)] * len(order)
    got = engine.merkle_continues_take(tree, order, wants, 3, None, caps=caps, retry=False)
    plain = engine.merkle_continues(tree, order, 3, None, caps=caps, retry=False)
    assert got[2] == plain[2] == ("error", _abi.DG_E_INVAL)
    assert got[-1][0] == "ok" and len(got[-1]) == 3 and got[-1][2] == 0
    for (rc, w), res, pl, wj in zip(hops, got[:2] + got[3:-1], plain[:2] + plain[3:-1], want):
        if B.kind_of(w) == "keys" and wj:
            assert_rows(engine, tree, rows_x, res, w[1])
        else:
            assert len(res) == len(pl) <= 3
            assert_same(res, pl)
            assert_is(res, w, 8)


def test_row_capacity_of_one_hop(engine):
    """One take a row short: its rc is DG_E_CAPACITY with the rows needed, its keys and the
    other hops' rows are right, and the retry at the reported size is exact."""
    rows_x, hops = x_hops("a", None)
    tree = side(engine, rows_x, 8)[0]
    conts = [dev_cont(rc, 8) for rc, _ in hops]
    want = [True] * len(hops)
    tried = 0
    for j, (_, w) in enumerate(hops):
        if B.kind_of(w) != "keys":
            continue
        need = int(expect_rows(rows_x, w[1])[1][-1])
        if need == 0:
            continue
        tried += 1
        caps = [None] * len(hops)
        caps[j] = need - 1
        got = engine.merkle_continues_take(tree, conts, want, 3, None, row_caps=caps, retry=False)
        assert got[j][0] == "ok" and np.array_equal(u64(got[j][1]), w[1]) and got[j][2] == len(w[1])
        assert got[j][3] is None and got[j][4] == ("capacity", need)
        for i, ((_, wi), res) in enumerate(zip(hops, got)):
            if i != j and B.kind_of(wi) == "keys":
                assert_rows(engine, tree, rows_x, res, wi[1])
        caps[j] = need
        exact = engine.merkle_continues_take(tree, conts, want, 3, None, row_caps=caps, retry=False)
        assert_rows(engine, tree, rows_x, exact[j], w[1])
        assert_rows(engine, tree, rows_x,
                    engine.merkle_continues_take(tree, conts, want, 3, None, row_caps=[0] * len(hops))[j], w[1])
    assert tried >= 2


@pytest.mark.parametrize("k", [1, 2, 64])
def test_batch_sizes(engine, k):
    rows_x, hops = x_hops("a", 200)
    start = next(j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "keys")
    batch = [hops[(start + i) % len(hops)] for i in range(k)]  # (k = 1: a keys hop)
    check_take(engine, side(engine, rows_x, 8)[0], rows_x, batch, 200, [True] * k)


def test_permuted_batch(engine):
    rows_x, hops = x_hops("a", None)
    hops = list(hops)
    random.Random(11).shuffle(hops)
    check_take(engine, side(engine, rows_x, 8)[0], rows_x, hops, None, [True] * len(hops))
    assert engine.merkle_continues_take(side(engine, rows_x, 8)[0], [], [], 3, None) == []


def test_arrival_word_and_sequence_across_calls(engine):
    """The arrival word and the sequence number are the plain call's: take, plain, the single
    hop, take in a row on one engine, all correct."""
    rows_x, hops = x_hops("a", None)
    tree = side(engine, rows_x, 8)[0]
    want = [True] * len(hops)
    check_take(engine, tree, rows_x, hops, None, want)
    for (rc, w), res in zip(hops, engine.merkle_continues(tree, [dev_cont(rc, 8) for rc, _ in hops], 3, None)):
        assert_is(res, w, 8)
    rc, w = hops[1]
    assert_is(engine.merkle_continue_home(tree, dev_cont(rc, 8), 3, None), w, 8)
    check_take(engine, tree, rows_x, [hops[i % len(hops)] for i in range(64)], None, [True] * 64)
    check_take(engine, tree, rows_x, hops[:3], None, want[:3])


def test_sharded_tree(engine):
    rows_x, hops = x_hops("a", None, 2, 1)
    assert "keys" in {B.kind_of(w) for _, w in hops}
    tree = side(engine, rows_x, 8, 2, 1)[0]
    conts = [dev_cont(rc, 8) for rc, _ in hops]
    got = engine.merkle_continues_take(tree, conts, [True] * len(hops), 3, None)
    for (_, w), res in zip(hops, got):
        if B.kind_of(w) == "keys":
            assert_rows(engine, tree, rows_x, res, w[1])
        else:
            assert_is(res, w, 8)
