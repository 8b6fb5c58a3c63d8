"""dgr_merkle_continue_batch through the NIF mirror (nif.merkle_continue_batch) on cuda:0: k
pending continuation messages answered in one call.  Element j must be byte for byte what
nif.merkle_continue returns for message j -- and what the C oracle answers -- whether the
launch, its capacity retry or the general calls served it.  The states hold the rows of
tests/partial_diff_cases.py by id (loaded through dgr_state_load: no term is interned, so the
trees hash the ids themselves and the oracle's trees are theirs)."""
import ctypes as C
import struct

import numpy as np
import pytest

import cont_batch_cases as B
import partial_diff_cases as P
from delta_crdt_ex_amd import _abi, nif

pytestmark = pytest.mark.gpu

LEVELS = 3


def frame(rc, depth):
    """the oracle's continuation as the message bytes (replica.h dgr_merkle_prepare)"""
    if rc[0] == "node":
        level, pos, hs, bk = int(rc[1]), rc[2], rc[3], np.zeros(0, np.uint64)
    else:
        level, bk, pos, hs = depth + 1, rc[1], rc[2], rc[3]
    words = [np.ascontiguousarray(x, np.uint64).tobytes() for x in (pos, hs, bk)]
    return struct.pack("<IQQ", level, len(pos), len(bk)) + b"".join(words)


def as_result(want, depth, max_sync=None):
    """the oracle's answer in nif.merkle_continue's shape: the first max_sync keys (Enum.take),
    as placeholders (no node interned them)"""
    if want[0] == "continue":
        return ("continue", frame(want[1], depth))
    return ("ok", [nif.key_placeholder(k) for k in want[1][:max_sync]])


@pytest.fixture(scope="module")
def eng():
    _ok, e = nif.engine_open(0)
    yield e
    e.close()


def load(eng, rows, depth):
    """a resident state of these rows (a VV over their four nodes) with its tree"""
    k, v, t, n, c = (np.ascontiguousarray(x) for x in rows)
    st = _abi.dg_store(k.ctypes.data, v.ctypes.data, t.ctypes.data, n.ctypes.data, c.ctypes.data, len(k), len(k))
    cn, cc = np.arange(4, dtype=np.uint32), np.full(4, 1 << 40, np.uint64)
    cx = _abi.dg_context(_abi.DG_CTX_VV, 0, cn.ctypes.data, cc.ctypes.data, 4, 4)
    ptr = C.c_void_p()
    assert eng.lib.dgr_state_load(eng.ptr, C.byref(st), C.byref(cx), C.byref(ptr)) == 0
    s = nif.State(eng, ptr)
    eng.states.append(s)
    assert nif.merkle_build(s, s.version, depth) == "ok"
    return s


@pytest.fixture(scope="module")
def ladder_x(eng):
    return load(eng, P.ladder(8)[0], 8)


@pytest.mark.parametrize("max_sync", [5, 200, "infinite"])
def test_each_element_is_the_single_call(eng, ladder_x, max_sync):
    """(Unbounded, the ladder's bucket-level hop answers 911 pairs for 176 buckets: more than the
    four per bucket it is first given, so the capacity retry serves it.)"""
    ms = None if max_sync == "infinite" else max_sync
    hops = B.ladder_hops(ms, LEVELS)
    assert {B.kind_of(w) for _, w in hops} == {"node", "leaf", "keys", "empty"}
    msgs = [frame(rc, 8) for rc, _ in hops]
    x, ver = ladder_x, ladder_x.version
    singles = [nif.merkle_continue(x, ver, m, LEVELS, max_sync) for m in msgs]
    assert singles == [as_result(w, 8, ms) for _, w in hops]
    assert nif.merkle_continue_batch(x, ver, msgs, LEVELS, max_sync) == ("ok", singles)
    assert nif.merkle_continue_batch(x, ver, [], LEVELS, max_sync) == ("ok", [])
    # more messages than one call takes: chunks of 64, in order
    many = [msgs[i % len(msgs)] for i in range(70)]
    assert nif.merkle_continue_batch(x, ver, many, LEVELS, max_sync) == (
        "ok", [singles[i % len(msgs)] for i in range(70)])
    assert x.version == ver  # answering moves no version


def test_a_message_over_the_limits_takes_the_general_path_alone(eng):
    """wide_pair() at depth 11, levels 4: the leaf form of 1448 buckets is over the launch's
    limits and is answered by the general calls, between hops the launch answers (among them
    the level-11 node form with 1448 buckets out)."""
    _, b = P.wide_pair()
    x = load(eng, b, 11)
    hops = B.wide_hops(11, 4)
    assert [P.over_home_limits(rc) for rc, _ in hops].count(True) == 1
    assert any(w[0] == "continue" and w[1][0] == "leaf" and len(w[1][1]) > 512 for _, w in hops)
    msgs = [frame(rc, 11) for rc, _ in hops]
    singles = [nif.merkle_continue(x, x.version, m, 4, "infinite") for m in msgs]
    assert singles == [as_result(w, 11) for _, w in hops]
    assert nif.merkle_continue_batch(x, x.version, msgs, 4, "infinite") == ("ok", singles)
    # a frame cut short is that element's error, as it is the single call's; the others stand
    cut = msgs[:1] + [msgs[1][:-8]] + msgs[2:]
    got = nif.merkle_continue_batch(x, x.version, cut, 4, "infinite")
    assert got[0] == "ok" and got[1][1][0] == "error" and got[1][1][1][0] == _abi.DG_E_INVAL
    assert nif.merkle_continue(x, x.version, cut[1], 4, "infinite")[0] == "error"
    assert got[1][:1] + got[1][2:] == singles[:1] + singles[2:]


def test_a_stale_version_fails_the_whole_call(eng, ladder_x):
    msgs = [frame(rc, 8) for rc, _ in B.ladder_hops(None, LEVELS)]
    assert nif.merkle_continue_batch(ladder_x, ladder_x.version + 1, msgs, LEVELS, "infinite") == ("error", "stale")
    assert nif.merkle_continue_batch(ladder_x, ladder_x.version, msgs[:2], LEVELS, "infinite")[0] == "ok"


@pytest.mark.parametrize("max_sync", [200, "infinite"])
def test_lockstep_conversations_with_four_neighbours(eng, ladder_x, max_sync):
    """X's four differing neighbours each prepare; the four conversations advance in lockstep to
    {:ok, keys}, X's pending messages answered hop by hop in one run and batched in the other.
    The keys each neighbour's conversation ends in are the same."""
    a, b, _ = P.ladder(8)
    cut = tuple(c[100:] for c in b)           # b without its first rows
    short = tuple(c[:-50] for c in a)         # X's rows without the last
    peers = [load(eng, r, 8) for r in (b, P.empty_rows(), cut, short)]
    x, ver = ladder_x, ladder_x.version

    def converse(batched):
        conts = {i: nif.merkle_prepare(p, p.version, LEVELS)[1] for i, p in enumerate(peers)}
        keys, rounds = {}, 0
        while conts:
            ids = sorted(conts)
            msgs = [conts[i] for i in ids]
            if batched:
                res = nif.merkle_continue_batch(x, ver, msgs, LEVELS, max_sync)
                assert res[0] == "ok"
                res = res[1]
            else:
                res = [nif.merkle_continue(x, ver, m, LEVELS, max_sync) for m in msgs]
            conts = {}
            for i, r in zip(ids, res):
                if r[0] == "continue":
                    r = nif.merkle_continue(peers[i], peers[i].version, r[1], LEVELS, max_sync)
                assert r[0] in ("ok", "continue"), r
                if r[0] == "ok":
                    keys[i] = r[1]
                else:
                    conts[i] = r[1]
            rounds += 1
            assert rounds <= 20, "the conversations do not end"
        return keys, rounds

    single, n1 = converse(False)
    batch, n2 = converse(True)
    assert n1 == n2 >= 2 and sorted(single) == [0, 1, 2, 3]
    assert batch == single
    assert all(len(single[i]) > 0 for i in range(4))
