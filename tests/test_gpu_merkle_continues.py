"""dg_merkle_continues on cuda:0 (csrc/merkle_cont.hip cont_hop_kernel<true>): the hops of k
neighbours' pending continuations in one launch, one workgroup per hop.  The answering
replica X is one side of tests/partial_diff_cases.py's pairs; a batch holds every continuation
X has to answer in its walks (tests/cont_batch_cases.py: both orientations, against the other
side, an empty replica and X itself).  Every hop of a batch is compared, in every field, with
the C oracle's continue_partial_diff + truncate_diff and with dg_merkle_continue_home on that
hop alone."""
import random

import numpy as np
import pytest
import torch

import cont_batch_cases as B
import partial_diff_cases as P
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd._abi import DeltaGpuError
from delta_crdt_ex_amd.store import MerkleCont, u64
from test_gpu_partial_diff import DEV, side

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).to(DEV)


def dev_cont(rc, depth):
    """the oracle's continuation as a device MerkleCont"""
    if rc[0] == "node":
        return MerkleCont(int(rc[1]), dev(rc[2]), dev(rc[3]), len(rc[2]))
    return MerkleCont(depth + 1, dev(rc[2]), dev(rc[3]), len(rc[2]), dev(rc[1]), len(rc[1]))


def assert_is(res, want, depth):
    """a hop's result against the oracle's answer"""
    assert res[0] == want[0], (res[0], want[0])
    if want[0] == "continue":
        P.assert_cont_equals(res[1], want[1], depth)
    else:
        assert res[2] == len(want[1])
        assert np.array_equal(u64(res[1]), want[1])


def assert_same(res, single):
    """a hop's result against dg_merkle_continue_home's for that hop alone, every field"""
    assert res[0] == single[0]
    if res[0] == "continue":
        c, s = res[1], single[1]
        assert (c.level, c.n, c.n_buckets) == (s.level, s.n, s.n_buckets)
        assert torch.equal(c.pos[: c.n], s.pos[: s.n]) and torch.equal(c.hash[: c.n], s.hash[: s.n])
        assert torch.equal(c.bucket[: c.n_buckets], s.bucket[: s.n_buckets])
    elif res[0] == "ok":
        assert res[2] == single[2] and torch.equal(res[1], single[1])
    else:
        assert res == single


def check_batch(engine, tree, hops, depth, levels, max_sync):
    """one batch, each hop against the oracle and against the single call"""
    conts = [dev_cont(rc, depth) for rc, _ in hops]
    got = engine.merkle_continues(tree, conts, levels, max_sync)
    assert len(got) == len(hops)
    for (rc, want), c, res in zip(hops, conts, got):
        single = engine.merkle_continue_home(tree, c, levels, max_sync)
        assert (single[0] == "declined") == P.over_home_limits(rc)
        assert_same(res, single)
        if res[0] != "declined":
            assert_is(res, want, depth)
    return got


@pytest.mark.parametrize("max_sync", [None, 5])
def test_parity_with_the_oracle_and_the_single_hop(engine, max_sync):
    a, _, _ = P.ladder(8)
    hops = B.ladder_hops(max_sync)
    assert {B.kind_of(w) for _, w in hops} == {"node", "leaf", "keys", "empty"}
    assert not any(P.over_home_limits(rc) for rc, _ in hops)
    check_batch(engine, side(engine, a, 8)[0], hops, 8, 3, max_sync)


def test_mixed_batch(engine):
    """A low node form, a bucket-level node form (1448 buckets out: more than one per thread),
    a leaf form in, an {:ok, []}, an empty input, a declined leaf form and a position outside
    the tree in one batch: the bad hop and the declined hop are reported as such, every other
    hop is its single-hop result."""
    _, b = P.wide_pair()
    tree = side(engine, b, 11)[0]
    hops = B.wide_hops(11, 4) + [h for h in B.wide_hops(11, 4, 200) if h[0][0] == "leaf"]
    declined = [P.over_home_limits(rc) for rc, _ in hops]
    assert sum(declined) == 1
    assert {B.kind_of(w) for (_, w), d in zip(hops, declined) if not d} == {"node", "leaf", "keys", "empty"}
    assert any(rc[0] == "node" and rc[1] == 11 and len(w[1][1]) > 512 for rc, w in hops if w[0] == "continue")
    conts = [dev_cont(rc, 11) for rc, _ in hops]
    bad = dev_cont(B.bad_position(hops[0][0]), 11)
    empty = dev_cont(B.empty_input(4), 11)
    order = conts[:2] + [bad] + conts[2:] + [empty]
    # (room for every answer at once: one dg_merkle_continues call, whose message is read below)
    got = engine.merkle_continues(tree, order, 4, None, caps=[(4 * 2048, 2048)] * len(order), retry=False)
    assert got[2] == ("error", _abi.DG_E_INVAL)
    assert b"hop 2: a position or bucket outside the tree" in engine.lib.dg_last_error()
    assert got[-1][0] == "ok" and got[-1][2] == 0 and got[-1][1].numel() == 0
    rest = got[:2] + got[3:-1]
    for (rc, want), c, res, d in zip(hops, conts, rest, declined):
        assert (res == ("declined",)) == d
        assert_same(res, engine.merkle_continue_home(tree, c, 4, None))
        if not d:
            assert_is(res, want, 11)


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_batch_sizes(engine, k):
    """k hops, the ladder's repeated to fill, each with outputs of its own"""
    a, _, _ = P.ladder(8)
    hops = B.ladder_hops(None)
    hops = [hops[i % len(hops)] for i in range(k)]
    tree = side(engine, a, 8)[0]
    got = engine.merkle_continues(tree, [dev_cont(rc, 8) for rc, _ in hops], 3, None)
    assert len(got) == k
    for (_, want), res in zip(hops, got):
        assert_is(res, want, 8)


def test_permuted_batch_and_the_bounds_of_k(engine):
    a, _, _ = P.ladder(8)
    hops = list(B.ladder_hops(None))
    random.Random(5).shuffle(hops)
    tree = side(engine, a, 8)[0]
    conts = [dev_cont(rc, 8) for rc, _ in hops]
    for (_, want), res in zip(hops, engine.merkle_continues(tree, conts, 3, None)):
        assert_is(res, want, 8)
    assert engine.merkle_continues(tree, [], 3, None) == []
    with pytest.raises(DeltaGpuError, match="65 hops"):
        engine.merkle_continues(tree, [conts[0]] * 65, 3, None)
    # a batch of hops that need no workgroup: empty inputs only
    got = engine.merkle_continues(tree, [dev_cont(B.empty_input(3), 8)] * 3, 3, None)
    assert all(r[0] == "ok" and r[2] == 0 for r in got)


def test_capacity_of_one_hop(engine):
    """One hop's output too small: it reports the sizes it needs, the others complete, and it
    succeeds alone at those sizes."""
    a, _, _ = P.ladder(8)
    hops = B.ladder_hops(None)
    tree = side(engine, a, 8)[0]
    conts = [dev_cont(rc, 8) for rc, _ in hops]
    roomy = (4096, 512)  # enough for every answer of the ladder
    for j, (_, want) in enumerate(hops):
        if want[0] != "continue":
            continue
        need = (len(want[1][2]), len(want[1][1]) if want[1][0] == "leaf" else 0)
        caps = [roomy] * len(hops)
        caps[j] = (need[0] - 1, max(need[1], 1))
        got = engine.merkle_continues(tree, conts, 3, None, caps=caps, retry=False)
        assert got[j] == ("capacity",) + need
        for i, ((_, w), res) in enumerate(zip(hops, got)):
            if i != j:
                assert_is(res, w, 8)
        assert_is(engine.merkle_continues(tree, [conts[j]], 3, None, caps=[need], retry=False)[0], want, 8)
        assert_is(engine.merkle_continues(tree, conts, 3, None, caps=caps)[j], want, 8)  # the wrapper's retry
    leaf = next(j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "leaf")
    want = hops[leaf][1]
    caps = [roomy] * len(hops)
    caps[leaf] = (len(want[1][2]), len(want[1][1]) - 1)  # one bucket short
    got = engine.merkle_continues(tree, conts, 3, None, caps=caps, retry=False)
    assert got[leaf] == ("capacity", len(want[1][2]), len(want[1][1]))


def test_large_branches_beside_small_hops(engine):
    """The 4096-entry node form (exactly the entry limit) and its 1900 buckets out, beside
    the walk's small hops; the declined leaf form of the same walk is declined here too."""
    _, b = P.wide_pair()
    hops = B.wide_hops(12, 8)
    assert any(len(rc[2]) == P.HOME_ENTRIES for rc, _ in hops)
    got = check_batch(engine, side(engine, b, 12)[0], hops, 12, 8, None)
    assert [r[0] for r in got].count("declined") == 1


def test_arrival_word_and_sequence_across_calls(engine):
    """k = 64, 1, 7 in a row on one engine, then a single hop, then a mutation through
    dg_join_delta_home (which waits on the same sequence word), then a batch again: an
    arrival word that was not reset or a sequence number that skipped fails one of them."""
    from test_gpu_home_diffs import _case, _setup
    from test_gpu_join_delta import kdev
    from test_gpu_parity import rows_eq
    a, _, _ = P.ladder(8)
    hops = B.ladder_hops(None)
    tree = side(engine, a, 8)[0]
    for k in (64, 1, 7):
        batch = [hops[i % len(hops)] for i in range(k)]
        got = engine.merkle_continues(tree, [dev_cont(rc, 8) for rc, _ in batch], 3, None)
        for (_, want), res in zip(batch, got):
            assert_is(res, want, 8)
    rc, want = hops[1]
    assert_is(engine.merkle_continue_home(tree, dev_cont(rc, 8), 3, None), want, 8)
    c, (wr, _wc, wch, _want, _cls) = _case("keys9", False)
    st, sc, sd, cd, spare, tr = _setup(engine, c, True)
    home = engine.join_delta_home(st, sc, sd, cd, kdev(c["keys"]), spare, tr)
    assert home is not None and np.array_equal(home[0], wch)
    rows_eq(st, wr)
    check_batch(engine, tree, hops, 8, 3, None)


def test_sharded_tree(engine):
    a, _, _ = P.ladder(8, 2, 1)
    hops = B.ladder_hops(None, 3, 2, 1)
    assert {B.kind_of(w) for _, w in hops} == {"node", "leaf", "keys", "empty"}
    check_batch(engine, side(engine, a, 8, 2, 1)[0], hops, 8, 3, None)
