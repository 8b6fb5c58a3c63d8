"""dg_join_delta_home_diffs on cuda:0: on_diffs' LWW reads of the changed keys out of the
one-launch join of a small delta (csrc/small.hip, small_delta_kernel<true>).  Every case of
home_diffs_cases.py (checked with the oracle alone by test_home_diffs_cases.py: which classes
of changed key each holds, and that it stays inside the small path's limits), with and
without a depth-12 tree, the delta's context as a dot set and as a VV:

  * words [0, DG_HOME_WORDS) of the block are bit for bit what dg_join_delta_home writes for
    the same input on a copy of the state (both blocks pre-filled with the same sentinel);
  * the state, its context and the tree equal dg_join_delta_rows' on a third copy;
  * the three arrays equal the C oracle's read/2 before and after its join on [0, n_changed),
    and nothing is written past them.

The cases: keysets of 1 and 8 keys (a wave searches each key), 9 (a thread does) and 512 (the
limit); every key keeping its row count (in place) and exactly one changing it (the spare
store and the tail kernel); a state above 131,072 rows (the splice after the wait); a winner
decided across the sign of ts; two values at the maximal ts before and after; a key of 1,000
state rows whose winner is the last one; 1,025 rows: DG_HOME_FALLBACK with everything --
the three ranges included -- untouched; a changed key whose read does not change; a key
removed and re-added by one delta; a key whose only delta row the state's VV covers."""
import numpy as np
import pytest
import torch

import home_diffs_cases as H
from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.store import Store, u64
from test_gpu_join_delta import _assert_unchanged, _snapshot, kdev, state_of, up
from test_gpu_parity import DEV, ctx_eq, rows_eq

pytestmark = pytest.mark.gpu

DEPTH = 12
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
_ORACLE = {}


def _case(name, vv):
    """the case and the oracle's answer, computed once and shared (read only)"""
    if (name, vv) not in _ORACLE:
        c = H.case(name, vv)
        _ORACLE[name, vv] = (c, H.oracle(c))
    return _ORACLE[name, vv]


def _setup(eng, c, with_tree):
    st, sc = state_of(c["a"], extra_ctx=len(c["d"]["ctx"][1]) + 4)
    sd, cd = up(c["d"])
    tree = eng.merkle_build(st, DEPTH) if with_tree else None
    return st, sc, sd, cd, Store.empty(st.n + sd.n, DEV), tree


def _same(p, q):
    for x, y in zip(p.to_numpy(), q.to_numpy()):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("vv", [False, True], ids=["dots", "vv"])
@pytest.mark.parametrize("with_tree", [False, True], ids=["no_tree", "tree"])
@pytest.mark.parametrize("name", [n for n in H.CASES if not H.CASES[n][3]])
def test_home_diffs(engine, name, with_tree, vv):
    c, (wr, wc, wch, want, cls) = _case(name, vv)
    keys = kdev(c["keys"])
    block = engine.home_block()
    W = _abi.DG_HOME_WORDS
    # the plain call on its own copy: the reference for the block's first DG_HOME_WORDS words
    st, sc, sd, cd, spare, tree = _setup(engine, c, with_tree)
    block[:] = SENTINEL
    plain = engine.join_delta_home(st, sc, sd, cd, keys, spare, tree)
    assert plain is not None, "the small path declined"
    plain_words = block[:W].copy()
    assert (block[W:] == SENTINEL).all()  # the plain call writes nothing behind its block
    # the diffs call
    st, sc, sd, cd, spare, tree = _setup(engine, c, with_tree)
    block[:] = SENTINEL
    got = engine.join_delta_home_diffs(st, sc, sd, cd, keys, spare, tree)
    assert got is not None, "the small path declined"
    assert np.array_equal(block[:W], plain_words)
    changed, hrows, hctx, swapped, (ov, nv, fl) = got
    assert swapped == c["moves"] == plain[3]
    assert np.array_equal(changed, wch)
    n = len(wch)
    for what, x, y in zip(("old_val", "new_val", "flags"), (ov, nv, fl), want):
        assert np.array_equal(x, y), (what, x[:8], y[:8])
    # nothing past the changed keys' entries
    assert (block[_abi.DG_HOME_DIFF_OLD + n:_abi.DG_HOME_DIFF_NEW] == SENTINEL).all()
    assert (block[_abi.DG_HOME_DIFF_NEW + n:_abi.DG_HOME_DIFF_FLAGS] == SENTINEL).all()
    assert (block[_abi.DG_HOME_DIFF_FLAGS:].view(np.uint8)[n:] == 0xA5).all()
    rows_eq(st, wr)
    ctx_eq(sc, wc)
    # dg_join_delta_rows on a third copy: the state, its context, the tree
    st2, sc2, sd2, cd2, spare2, tree2 = _setup(engine, c, with_tree)
    rows2 = Store.empty(st2.n + sd2.n, DEV)
    changed2, swapped2 = engine.join_delta(st2, sc2, sd2, cd2, keys, spare2, tree2, rows=rows2)
    assert swapped2 == swapped and np.array_equal(u64(changed2), changed)
    _same(st, st2)
    _same(sc, sc2)
    if with_tree:
        assert torch.equal(tree.nodes, tree2.nodes) and torch.equal(tree.counts, tree2.counts)
        assert torch.equal(tree.starts, tree2.starts) and tree.n_keys == tree2.n_keys
    for k in c["must"]:
        assert cls[k] >= 1


@pytest.mark.parametrize("vv", [False, True], ids=["dots", "vv"])
@pytest.mark.parametrize("with_tree", [False, True], ids=["no_tree", "tree"])
def test_home_diffs_fallback_touches_nothing(engine, with_tree, vv):
    """1,025 state rows under the keyset (SMALL_TAKEN is 1,024): DG_HOME_FALLBACK; the state,
    its context, the tree and the three diff ranges (pre-filled) are byte for byte what they
    were, and the general path then serves the same call."""
    c, (wr, wc, wch, want, cls) = _case("deep_over", vv)
    st, sc, sd, cd, spare, tree = _setup(engine, c, with_tree)
    rows0, ctx0 = [x.copy() for x in st.to_numpy()], [x.copy() for x in sc.to_numpy()]
    snap = _snapshot(st, sc, tree) if with_tree else None
    block = engine.home_block()
    block[:] = SENTINEL
    assert engine.join_delta_home_diffs(st, sc, sd, cd, kdev(c["keys"]), spare, tree) is None
    assert int(block[0]) & _abi.DG_HOME_FALLBACK
    assert (block[_abi.DG_HOME_DIFF_OLD:] == SENTINEL).all()
    for x, y in zip(st.to_numpy(), rows0):
        assert np.array_equal(x, y)
    for x, y in zip(sc.to_numpy(), ctx0):
        assert np.array_equal(x, y)
    if with_tree:
        _assert_unchanged(st, sc, tree, snap)
    changed, ov, nv, fl, _ = engine.join_delta_diffs(st, sc, sd, cd, kdev(c["keys"]), spare, tree)
    assert np.array_equal(u64(changed), wch)
    for x, y in zip((u64(ov), u64(nv), fl.cpu().numpy()), want):
        assert np.array_equal(x, y)
    rows_eq(st, wr)
