"""The generator of the dg_mutate_home cases (mutate_home_cases.py) checked with the C oracle
alone, no GPU: every case contains by construction what it is for (`must`), the cases the GPU
test expects to be served are inside the call's limits and the others just outside one of
them, and the rows move exactly where the case says."""
import numpy as np
import pytest

import mutate_home_cases as H
from lww_diffs_cases import NEW, OLD


def _run_lengths(rows, keys):
    return np.searchsorted(rows[0], keys, "right") - np.searchsorted(rows[0], keys, "left")


def _holds(c, o):
    """What a case contains, by name."""
    a, node, ops = c["a"], c["node"], c["ops"]
    rows, (_, vn, vc) = a["rows"], a["ctx"]
    wr, wch, touched = o["rows"], o["changed"], o["touched"]
    ov, nv, fl = o["diffs"]
    vv = {int(n): int(x) for n, x in zip(vn, vc)}
    c0 = vv.get(node, 0)
    na, ne = _run_lengths(rows, touched), _run_lengths(wr, touched)
    sel = np.isin(rows[0], touched)
    both = fl == OLD | NEW
    last = {}
    for kind, key, _, _ in ops:
        last.setdefault(key, []).append(kind)
    pairs = {(k[-2], k[-1]) for k in last.values() if len(k) >= 2}
    n_adds = sum(1 for op in ops if op[0] == H.A)
    uncovered = [(int(n), int(x)) for n, x in zip(rows[3][sel], rows[4][sel]) if vv.get(int(n), 0) < int(x)]
    old_ts = {int(k): t for k, t in zip(rows[0], rows[2])}  # (one-row keys: the row's ts)
    new_ts = {int(k): t for k, t in zip(o["delta"][0], o["delta"][2])}
    # a state row equal in all five columns to a delta row
    srows = set(zip(*[x[sel].tolist() for x in rows]))
    drows = set(zip(*[x.tolist() for x in o["delta"]]))
    return {
        "added": bool((fl == NEW).any()),
        "removed": bool((fl == OLD).any()),
        "updated": bool((both & (ov != nv)).any()),
        "unchanged_read": bool((both & (ov == nv)).any()),
        "silent": len(wch) < len(touched),
        "ctx_unchanged": n_adds == 0 and all(np.array_equal(x, y) for x, y in zip(a["ctx"], o["ctx"])),
        "in_place": bool((na == ne).all()),
        "one_moves": int((na != ne).sum()) == 1,
        "three_nodes": any(len(set(rows[3][rows[0] == k].tolist())) == 3 for k in touched),
        # an overwritten add's rank is consumed: a row of the joined state carries a later dot
        "rank_consumed": bool(((wr[3] == node) & (wr[4] > c0 + 1) & np.isin(wr[0], touched)).any())
        and any(k.count(H.A) >= 2 or (H.A, H.RM) in zip(k, k[1:]) for k in last.values()),
        "pairs": pairs >= {(H.A, H.A), (H.A, H.RM), (H.RM, H.A), (H.RM, H.RM)},
        "neg_ts": any((old_ts[k] < 0) != (new_ts[k] < 0) for k in new_ts if k in old_ts),
        "uncovered": bool(uncovered) and all(dict(zip(o["ctx"][1].tolist(), o["ctx"][2].tolist())).get(n, 0) >= x
                                             for n, x in uncovered),
        "in_both": bool(srows & drows),
        "node_absent": node not in vv,
        "node70": node == 70,
        "node2047": node == H.MAX_NODES - 1,
        "node2048": node == H.MAX_NODES,
        "large": len(rows[0]) > 131_072 and bool((na != ne).any()),
        "ops512": len(ops) == H.MAX_OPS,
        "ops513": len(ops) == H.MAX_OPS + 1,
        "keys3": len(touched) == 3,
        "taken1024": int(na.sum()) == H.MAX_TAKEN,
        "taken1025": int(na.sum()) == H.MAX_TAKEN + 1,
        "dots_over_1024": len(o["dots"][1]) > 1024 and int(na.sum()) <= H.MAX_TAKEN,
    }


@pytest.mark.parametrize("name", list(H.CASES))
def test_case_contains_what_it_is_for(name):
    c = H.case(name)
    o = H.oracle(c)
    holds = _holds(c, o)
    for k in c["must"]:
        assert holds[k], (name, k)
    a, touched = c["a"], o["touched"]
    assert len(touched) == len(c["recipes"]) == len(set(c["keys"].tolist()))
    # batch order is not key order wherever there are enough keys to tell
    if len(touched) >= 8:
        first = [op[1] for op in c["ops"][: len(touched)]]
        assert first != sorted(first)
    # the limits of the call: ops, taken rows, node ids, no counter at the maximum
    taken = int(_run_lengths(a["rows"], touched).sum())
    nodes = np.concatenate([a["ctx"][1], a["rows"][3][np.isin(a["rows"][0], touched)], [c["node"]]])
    inside = len(c["ops"]) <= H.MAX_OPS and taken <= H.MAX_TAKEN and int(nodes.max()) < H.MAX_NODES
    assert inside == c["served"], (name, len(c["ops"]), taken, int(nodes.max()))
    if c["served"]:
        moved = bool((_run_lengths(a["rows"], touched) != _run_lengths(o["rows"], touched)).any())
        assert moved == c["moves"], name
    for n, want in (("state0", 0), ("state1", 1), ("state64", 64), ("state65", 65)):
        if name == n:
            assert len(a["rows"][0]) == want


def test_marshal_sorts_stably_and_ranks_in_batch_order():
    c = H.case("every")
    kind, key, val, ts, rank, n_adds = H.marshal(c["ops"])
    assert np.all(np.diff(key.astype(np.float64)) >= 0) and n_adds == int(kind.sum())
    for k in np.unique(key):  # batch order within a key
        mine = [(1 if op[0] == H.A else 0, op[2], op[3]) for op in c["ops"] if op[1] == k]
        got = [(int(a), int(b), int(x)) for a, b, x in zip(kind[key == k], val[key == k], ts[key == k])]
        assert mine == got
    assert sorted(rank[kind == 1].tolist()) == list(range(n_adds))
    r = 0
    for op in c["ops"]:  # an add's rank: the adds before it in the batch
        if op[0] == H.A:
            i = np.flatnonzero((key == np.uint64(op[1])) & (val == np.uint64(op[2])) & (kind == 1))
            assert r in rank[i].tolist()
            r += 1


def test_recipes_read_what_they_say():
    """Known answers (read/2 before and after) for the recipes of `every`."""
    c = H.case("every")
    o = H.oracle(c)
    ov, nv, fl = o["diffs"]
    by = {}
    for name, key in zip(c["recipes"], c["keys"]):
        i = np.flatnonzero(o["changed"] == key)
        by[name] = (int(ov[i[0]]), int(nv[i[0]]), int(fl[i[0]])) if len(i) else None
    assert by["absent_add"] == (0, 52, NEW)
    assert by["update1"] == (53, 70, OLD | NEW)
    assert by["update3"] == (41, 71, OLD | NEW)
    assert by["remove"] == (51, 0, OLD)
    assert by["absent_remove"] is None
    assert by["aa"] == (55, 81, OLD | NEW) and by["ra"] == (55, 83, OLD | NEW)
    assert by["ar"] == (55, 0, OLD) and by["rr"] == (55, 0, OLD)
    assert by["neg_new"] == (56, 57, OLD | NEW) and by["neg_old"] == (58, 59, OLD | NEW)
    assert by["same_value"] == (54, 54, OLD | NEW)
    assert by["uncovered"] == (60, 61, OLD | NEW)
    assert by["in_both"] is None
