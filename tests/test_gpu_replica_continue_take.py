"""dgr_merkle_continue_take_batch through the NIF mirror (nif.merkle_continue_take_batch) on
cuda:0: k pending continuation messages answered in one call, the {:ok, keys} answers of the
messages that want it with Map.take(value, keys) beside them.  Element j must be what the two
existing calls give -- nif.merkle_continue for the answer, nif.take of its keys for the value
map -- whether the rows came out of the launch or through the fallback.  States are loaded as
tests/test_gpu_replica_continue_batch.py loads them."""
import ctypes as C

import numpy as np
import pytest

import cont_batch_cases as B
import partial_diff_cases as P
import take_pass_cases as T
from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd import workloads as W
from test_gpu_replica_continue_batch import frame, load

pytestmark = pytest.mark.gpu

LEVELS = 3


@pytest.fixture(scope="module")
def eng():
    _ok, e = nif.engine_open(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ladder_x(eng):
    return load(eng, P.ladder(8)[0], 8)


def _cols(st):
    n = int(st.n)
    return [nif._arr(p, n, dt).tolist() for p, dt in ((st.key, np.uint64), (st.val, np.uint64), (st.ts, np.int64),
                                                      (st.node, np.uint32), (st.cnt, np.uint64))]


def take_batch(x, ver, msgs, want, levels, max_sync):
    """dgr_merkle_continue_take_batch as nif.merkle_continue_take_batch calls it, with the rows as
    their five columns and the offsets instead of terms (these states intern no term): per message
    ("continue", bytes) | ("ok", key ids) | ("ok", key ids, columns, offs)"""
    eng = x.engine
    assert eng.refresh_terms() == 0
    mx = nif.U64_MAX if max_sync == "infinite" else int(max_sync)
    out = []
    for c0 in range(0, len(msgs), nif.CONT_BATCH_MAX):
        chunk = msgs[c0:c0 + nif.CONT_BATCH_MAX]
        k = len(chunk)
        res, taken = (nif.dgr_cont_result * max(k, 1))(), (nif.dgr_hop_rows * max(k, 1))()
        rc = eng.lib.dgr_merkle_continue_take_batch(
            x.ptr, ver, k, (C.c_char_p * max(k, 1))(*chunk), (C.c_uint64 * max(k, 1))(*[len(c) for c in chunk]),
            bytes(1 if w else 0 for w in want[c0:c0 + k]), levels, mx, res, taken)
        if rc:
            return rc
        for r, t in zip(res[:k], taken[:k]):
            assert r.rc == 0
            if r.status == 1:
                out.append(("continue", C.string_at(r.bin, r.len)))
            elif t.offs:
                out.append(("ok", nif._arr(r.keys, r.n_keys, np.uint64).tolist(), _cols(t.rows),
                            nif._arr(t.offs, r.n_keys + 1, np.uint64).tolist()))
            else:
                assert t.rows.n == 0
                out.append(("ok", nif._arr(r.keys, r.n_keys, np.uint64).tolist()))
    return out


def two_calls(x, ver, msgs, want, levels, max_sync):
    """(merkle_continue(msg), dgr_take(keys)) by the existing calls, in take_batch's shape"""
    out = []
    for m, w in zip(msgs, want):
        r = nif.merkle_continue(x, ver, m, levels, max_sync)
        if r[0] == "ok":
            keys = [int(k[1]) for k in r[1]]  # (placeholders: no term is interned)
            r = ("ok", keys)
            if w and keys:
                st = _abi.dg_store()
                ka = np.array(keys, np.uint64)
                assert x.engine.lib.dgr_take(x.ptr, ver, ka.ctypes.data, len(ka), C.byref(st)) == 0
                cols = _cols(st)
                offs = np.concatenate([np.searchsorted(np.array(cols[0], np.uint64), ka, "left"),
                                       [len(cols[0])]]).tolist()
                r = ("ok", keys, cols, offs)
        out.append(r)
    return out


@pytest.mark.parametrize("max_sync", [5, 200, "infinite"])
def test_each_element_is_the_two_calls(eng, ladder_x, max_sync):
    ms = None if max_sync == "infinite" else max_sync
    hops = B.ladder_hops(ms, LEVELS)
    assert {B.kind_of(w) for _, w in hops} == {"node", "leaf", "keys", "empty"}
    msgs = [frame(rc, 8) for rc, _ in hops]
    x, ver = ladder_x, ladder_x.version
    for want in ([True] * len(msgs), [False] * len(msgs), [j % 2 == 0 for j in range(len(msgs))],
                 [j % 2 == 1 for j in range(len(msgs))]):
        exp = two_calls(x, ver, msgs, want, LEVELS, max_sync)
        got = take_batch(x, ver, msgs, want, LEVELS, max_sync)
        assert got == exp
        assert any(len(e) == 4 and e[2][0] for e in exp) == any(
            w and B.kind_of(h[1]) == "keys" for w, h in zip(want, hops))
    assert nif.merkle_continue_take_batch(x, ver, msgs, [False] * len(msgs), LEVELS, max_sync) == \
        nif.merkle_continue_batch(x, ver, msgs, LEVELS, max_sync)
    assert nif.merkle_continue_take_batch(x, ver, [], [], LEVELS, max_sync) == ("ok", [])
    many = [msgs[i % len(msgs)] for i in range(70)]  # chunks of 64, in order
    exp = two_calls(x, ver, msgs, [True] * len(msgs), LEVELS, max_sync)
    assert take_batch(x, ver, many, [True] * 70, LEVELS, max_sync) == [exp[i % len(msgs)] for i in range(70)]
    assert x.version == ver


def test_general_path_rows(eng):
    """wide_pair() at depth 11, levels 4: the leaf form of 1448 buckets is over the launch's limits
    and is answered by the general calls; its rows come through the fallback and are exact."""
    _, b = P.wide_pair()
    x = load(eng, b, 11)
    hops = B.wide_hops(11, 4)
    assert sum(P.over_home_limits(rc) for rc, _ in hops) == 1
    msgs = [frame(rc, 11) for rc, _ in hops]
    want = [True] * len(msgs)
    exp = two_calls(x, x.version, msgs, want, 4, "infinite")
    over = next(j for j, (rc, _) in enumerate(hops) if P.over_home_limits(rc))
    assert len(exp[over]) == 4 and len(exp[over][2][0]) > 512
    assert take_batch(x, x.version, msgs, want, 4, "infinite") == exp


@pytest.mark.parametrize("max_sync", ["infinite", T.CUTS[0]])
def test_multi_pass_rows_out_of_the_launch(eng, max_sync):
    """take_pass_cases.stairs() at depth 9: keys hops of more than 4096 rows, which the launch
    copies in several passes.  That the launch and not the fallback take serves them is the room
    rule of replica_pack.h, restated: a hop has room for min(rows_n, 4 * min(kcap, 4096) + 64) rows,
    kcap = min(max_sync, rows_n + n + 1, 65536).  Unbounded that is all 16,440 rows of X, which the
    hop against the empty replica needs (five passes, the 8200-row key among them).  At the cut
    the 8200-row key alone is over four rows a key, so it is kept out of the hop meant here: the
    hop against the empty replica, cut before that key, needs 4760 rows of its 9052 (two passes),
    while the hop against P, which holds the key, is over its room and comes through the
    fallback beside it."""
    ms = None if max_sync == "infinite" else max_sync
    rows_x, _ = T.stairs()
    hops = T.hops_of_conversations(ms)
    keys_hops = [(rc, T.kept_of(w, ms)) for rc, w in hops if B.kind_of(w) == "keys"]
    need = [T.row_total(rows_x, kept) for _, kept in keys_hops]
    room = [min(len(rows_x[0]), 4 * min(min(len(rows_x[0]) + len(rc[2]) + 1, 65536, *([ms] if ms else [])), 4096) + 64)
            for rc, _ in keys_hops]
    assert room == [T.replica_room(len(rows_x[0]), len(rc[2]), ms) for rc, _ in keys_hops]
    served = [n for n, r in zip(need, room) if n <= r]
    assert max(served) > 4096 and (ms is not None or max(served) == max(need) == len(rows_x[0]))
    x = load(eng, rows_x, T.DEPTH)
    msgs = [frame(rc, T.DEPTH) for rc, _ in hops]
    want = [True] * len(msgs)
    exp = two_calls(x, x.version, msgs, want, T.LEVELS, max_sync)
    assert sorted(len(e[2][0]) for e in exp if len(e) == 4) == sorted(need)
    assert take_batch(x, x.version, msgs, want, T.LEVELS, max_sync) == exp


def overflow_pair():
    """X holds three keys of 40 rows each in different buckets of a depth-8 tree (0, 1 and 2: one
    level-6 node, so the truncation of every hop to 5 entries keeps all three); the peer holds the
    same rows with one ts bumped per key: 120 rows for 3 keys against a room of 4 * 5 + 64 = 84."""
    key = np.repeat((np.array([0, 1, 2], np.uint64) << np.uint64(56)) + np.uint64(16), 40)
    n = len(key)
    rng = np.random.default_rng(40)
    val = np.uint64(1 << 62) + rng.integers(0, 1 << 20, n).astype(np.uint64)
    ts = rng.integers(0, 1 << 40, n).astype(np.int64)
    node = rng.integers(0, 4, n).astype(np.uint32)
    cnt = np.arange(1, n + 1, dtype=np.uint64)
    a = W.sort_rows(key, val, ts, node, cnt)
    tb = a[2].copy()
    tb[[0, 40, 80]] += 1
    return a, W.sort_rows(a[0], a[1], tb, a[3], a[4])


def test_row_room_overflow_falls_back(eng):
    a, b = overflow_pair()
    x = load(eng, a, 8)
    hops = B.hops_of(a, (b,), 8, LEVELS, 5)
    keys_hops = [j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "keys"]
    assert keys_hops and all(len(hops[j][1][1]) == 3 for j in keys_hops)
    assert int(np.isin(a[0], hops[keys_hops[0]][1][1]).sum()) == 120 > 4 * 5 + 64
    msgs = [frame(rc, 8) for rc, _ in hops]
    want = [True] * len(msgs)
    exp = two_calls(x, x.version, msgs, want, LEVELS, 5)
    assert max(len(e[2][0]) for e in exp if len(e) == 4) == 120
    assert take_batch(x, x.version, msgs, want, LEVELS, 5) == exp
    # twice in one batch: both hops fall back through the one take
    assert take_batch(x, x.version, msgs + msgs, want + want, LEVELS, 5) == exp + exp


def test_lone_hop_and_stale_version(eng, ladder_x):
    hops = B.ladder_hops(200, LEVELS)
    j = next(j for j, (_, w) in enumerate(hops) if B.kind_of(w) == "keys")
    msg = frame(hops[j][0], 8)
    x, ver = ladder_x, ladder_x.version
    exp = two_calls(x, ver, [msg], [True], LEVELS, 200)
    assert len(exp[0]) == 4 and exp[0][2][0]
    assert take_batch(x, ver, [msg], [True], LEVELS, 200) == exp
    node = frame(hops[0][0], 8)  # a lone node form: the single call, no rows
    assert nif.merkle_continue_take_batch(x, ver, [node], [True], LEVELS, 200) == \
        ("ok", [nif.merkle_continue(x, ver, node, LEVELS, 200)])
    assert nif.merkle_continue_take_batch(x, ver + 1, [msg], [True], LEVELS, 200) == ("error", "stale")
    assert take_batch(x, ver + 1, [msg], [True], LEVELS, 200) == nif.DGR_E_STALE
    assert x.version == ver


def test_value_maps_of_interned_states(eng):
    """Through terms: two states loaded with their terms, the conversation run through the NIF
    mirror; the messages X receives answered by the one call equal merkle_continue + take."""
    def value(bumped):
        return {("k", i): {(("v", i % 5), 1000 + i + (1 if i in bumped else 0)): {("n", i % 3 + 1), ("m", i + 1)}}
                for i in range(300)}
    dots = {"n": 4, "m": 301}
    _ok, x, vx = nif.state_load(eng, dots, value(()))
    _ok, p, vp = nif.state_load(eng, dots, value(range(0, 300, 7)))
    assert nif.merkle_build(x, vx, 8) == "ok" and nif.merkle_build(p, vp, 8) == "ok"
    msg, mine, inbox = nif.merkle_prepare(x, vx, 3)[1], False, []
    for _ in range(12):
        if mine:
            inbox.append(msg)
        r = nif.merkle_continue(x if mine else p, vx if mine else vp, msg, 3, 200)
        if r[0] == "ok":
            assert mine and len(r[1]) == len(range(0, 300, 7))
            break
        msg, mine = r[1], not mine
    exp = []
    for m in inbox:
        r = nif.merkle_continue(x, vx, m, 3, 200)
        exp.append(("ok", r[1], nif.take(x, vx, r[1])[1]) if r[0] == "ok" and r[1] else r)
    assert len(exp[-1]) == 3 and len(exp[-1][2]) == len(exp[-1][1])
    assert nif.merkle_continue_take_batch(x, vx, inbox, [True] * len(inbox), 3, 200) == ("ok", exp)
    assert nif.merkle_continue_take_batch(x, vx, inbox[-1:], [True], 3, 200) == ("ok", exp[-1:])
    assert nif.merkle_continue_take_batch(x, vx, inbox, [False] * len(inbox), 3, 200) == \
        nif.merkle_continue_batch(x, vx, inbox, 3, 200)
