"""dg_merkle_continues_take on cuda:0 past one staging pass (csrc/merkle_cont.hip take_hop): hops
whose kept keys own more than CS_IN = 4096 rows, so that the pass loop runs two to five times,
keys straddle, end at and start at the pass boundaries in both walks (walk_taken over register
buckets, walk_global over big ones), and the rows' store indices differ from their output
indices; and the block scan's row total at 2^22 - 1, 2^22 and 2^22 + 1, where it changes from
one 32-bit scan to the scans of two 16-bit halves.

The inputs are tests/take_pass_cases.py's (tests/test_take_pass_cases.py proves on the CPU that
the cases below reach every situation it names; the largest take, all of X, is five passes).
Every comparison is exact: keys against the C oracle, rows and offsets against numpy's selection
of X's sorted rows and against take_keys, every other element against merkle_continues.

Not checked: rows written for a total of 2^22 or more.  huge()'s hops are given room for 4096
rows and no retry, so only the scans' total (the rows needed) and the keys are compared; the
per-thread offset the halves scan yields is never used to write a row here."""
import numpy as np
import pytest
import torch

import cont_batch_cases as B
import take_pass_cases as T
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.store import Store, u64
from test_gpu_merkle_continues import assert_is, dev_cont
from test_gpu_merkle_continues_take import assert_rows, check_take
from test_gpu_partial_diff import DEV, side

pytestmark = pytest.mark.gpu

D = T.DEPTH


def stairs_tree(engine):
    rows_x, _ = T.stairs()
    return rows_x, side(engine, rows_x, D)[0]


def keys_hop(hops, rows_x, total):
    """the index of the first keys hop whose keys own exactly `total` rows of X"""
    return next(j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "keys" and T.row_total(rows_x, w[1]) == total)


@pytest.mark.parametrize("max_sync", T.CASES)
def test_parity_with_the_two_calls(engine, max_sync):
    rows_x, tree = stairs_tree(engine)
    hops = T.hops(max_sync)
    got = check_take(engine, tree, rows_x, hops, max_sync, [True] * len(hops), depth=D)
    assert any(len(r) == 5 and r[4].n > 2 * T.PASS for r in got)


def test_batch_of_64(engine):
    """Sixty-four workgroups copying at once, most of them over several passes: the hops of the
    unbounded cases in turn (node forms, a leaf out, the one-pass hop of 4096 rows next to the
    four-pass hop), one keys hop without a take and a position outside the tree.  The bad hop is
    reported alone; every other element is exact."""
    rows_x, tree = stairs_tree(engine)
    hops = T.hops(None)
    batch = [hops[i % len(hops)] for i in range(64)]
    totals = [T.row_total(rows_x, w[1]) if B.kind_of(w) == "keys" else None for _, w in batch]
    assert any(a == T.PASS and b is not None and 3 * T.PASS < b <= 4 * T.PASS for a, b in zip(totals, totals[1:]))
    plain = next(j for j in range(32, 64) if totals[j] is not None and totals[j] > T.PASS)
    bad = next(j for j in range(32, 64) if batch[j][0][0] == "node")
    assert any(rc[0] == "node" for j, (rc, _) in enumerate(batch) if j != bad)
    conts = [dev_cont(rc, D) for rc, _ in batch]
    conts[bad] = dev_cont(B.bad_position(batch[bad][0]), D)
    want = [j != plain for j in range(64)]
    got = engine.merkle_continues_take(tree, conts, want, T.LEVELS, None)
    assert len(got) == 64 and got[bad] == ("error", _abi.DG_E_INVAL)
    for j, ((_, w), res) in enumerate(zip(batch, got)):
        if j == bad:
            continue
        if B.kind_of(w) == "keys" and j != plain:
            assert res[2] == len(w[1])
            assert_rows(engine, tree, rows_x, res, w[1])
        else:
            assert len(res) <= 3
            assert_is(res, w, D)


@pytest.mark.parametrize("total", [2 * T.PASS, T.PASS + 1])
def test_row_capacity_at_a_pass_boundary(engine, total):
    """Room for one row fewer than a hop of 8192 (4097) rows needs -- 8191: two passes all but a
    row; 4096: one whole pass -- is DG_E_CAPACITY with the rows needed and the keys right, the
    other takes of the batch exact; room for exactly the rows is exact."""
    rows_x, tree = stairs_tree(engine)
    hops = T.hops(None)
    j = keys_hop(hops, rows_x, total)
    conts = [dev_cont(rc, D) for rc, _ in hops]
    want = [True] * len(hops)
    caps = [None] * len(hops)
    caps[j] = total - 1
    got = engine.merkle_continues_take(tree, conts, want, T.LEVELS, None, row_caps=caps, retry=False)
    w = hops[j][1]
    assert got[j][0] == "ok" and np.array_equal(u64(got[j][1]), w[1]) and got[j][2] == len(w[1])
    assert got[j][3] is None and got[j][4] == ("capacity", total)
    for i, ((_, wi), res) in enumerate(zip(hops, got)):
        if i != j and B.kind_of(wi) == "keys":
            assert_rows(engine, tree, rows_x, res, wi[1])
    caps[j] = total
    exact = engine.merkle_continues_take(tree, conts, want, T.LEVELS, None, row_caps=caps, retry=False)
    assert_rows(engine, tree, rows_x, exact[j], w[1])


def test_nothing_written_past_the_rows(engine, monkeypatch):
    """A three-pass hop (against P: 11,176 rows, every one at a store index above its output
    index) given room for 64 rows more than it needs: the 64 rows past the last are untouched in
    all five columns.  The canvas is pre-filled: Store.empty is replaced, for this test, by one
    that fills what it allocates with a pattern and waits for the fill, so the check needs neither
    a second run to compare with nor rests on rows.n alone."""
    rows_x, tree = stairs_tree(engine)
    hops = T.hops(None)
    rc, w = next(h for h in hops if B.kind_of(h[1]) == "keys")  # the conversation with P ends in it
    need = T.row_total(rows_x, w[1])
    assert 2 * T.PASS < need < len(rows_x[0]) and "shifted" in T.key_paths(rows_x, tree.bucket_counts(), w[1], None)
    empty, fill = Store.empty, -0x0123456789abcdef

    def filled(cap, device):
        s = empty(cap, device)
        for c in (s.key, s.val, s.ts, s.cnt):
            c.fill_(fill)
        s.node.fill_(fill & 0x7fffffff)
        torch.cuda.synchronize()
        return s

    monkeypatch.setattr(Store, "empty", staticmethod(filled))
    res = engine.merkle_continues_take(tree, [dev_cont(rc, D)], [True], T.LEVELS, None, row_caps=[need + 64],
                                       retry=False)[0]
    monkeypatch.undo()
    assert_rows(engine, tree, rows_x, res, w[1])
    rows = res[4]
    assert rows.n == need and rows.cap == need + 64
    for c in (rows.key, rows.val, rows.ts, rows.cnt):
        assert torch.all(c[need:] == fill) and not torch.any(c[:need] == fill)
    assert torch.all(rows.node[need:] == fill & 0x7fffffff)


@pytest.fixture(scope="module")
def huge_tree(engine):
    rows = T.huge()
    tree = engine.merkle_build(Store.from_numpy(*rows, device=DEV), D)
    counts = np.bincount((rows[0] >> np.uint64(T.SHIFT)).astype(np.int64), minlength=T.NBK)
    assert tree.n_keys == 1025 and np.array_equal(tree.bucket_counts(), counts)
    yield rows, tree
    del tree
    torch.cuda.empty_cache()


def test_scan_totals_around_2_pow_22(engine, huge_tree):
    """The leaf form of all 512 buckets with no pairs against huge(): every key differs, and the
    first 1023, 1024 and all 1025 of them own 2^22 - 1, 2^22 and 2^22 + 1 rows: the last total of
    the 32-bit scan, the first of the halves scan and the one after.  Each hop has room for 4096
    rows and is not retried (writing 2^22 rows would be a thousand passes over 8193-row buckets):
    its element is the keys and ("capacity", rows needed).  max_sync is the call's, not a hop's,
    so the three cuts are three calls, each of them the hop three times over."""
    rows, tree = huge_tree
    cont = T.huge_cont()
    for max_sync, total in zip(T.HUGE_CUTS, ((1 << 22) - 1, 1 << 22, (1 << 22) + 1)):
        kept, n_keys, need = T.huge_expect(rows, max_sync)
        assert need == total
        got = engine.merkle_continues_take(tree, [dev_cont(cont, D)] * 3, [True] * 3, T.LEVELS, max_sync,
                                           row_caps=[T.PASS] * 3, retry=False)
        assert len(got) == 3
        for res in got:
            assert len(res) == 5 and res[0] == "ok" and res[2] == n_keys
            assert np.array_equal(u64(res[1]), kept)
            assert res[3] is None and res[4] == ("capacity", need)
