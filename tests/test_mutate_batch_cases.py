"""The generator of the dg_mutate_batch cases (mutate_batch_cases.py) checked with the oracle
alone, no GPU: every case holds what its name says -- the tile count, which sorted positions
open and close a group at the tile seam, the empty dot lists, the add count that makes the
generator's grid go round, the node's place in the VV, the wide dots under the touched keys --
so a case that lost its point fails here instead of passing on the GPU."""
import numpy as np
import pytest

import mutate_batch_cases as M
from mutate_batch_cases import A, RM

_CACHE = {}


def _case(name):
    if name not in _CACHE:
        c = M.case(name)
        _CACHE[name] = (c, M.oracle(c, join=False))
    return _CACHE[name]


def _sorted(c):
    """the marshalled batch and, per sorted position, whether it opens / closes its group"""
    kind, key, val, ts, rank, n_adds = M.marshal(c["ops"])
    head = np.r_[True, key[1:] != key[:-1]]
    last = np.r_[key[1:] != key[:-1], True]
    return kind, key, val, ts, rank, n_adds, head, last


def _counts(c, o):
    """(m, n_adds, state dots under the touched keys, dots of the oracle's list)"""
    n_adds = sum(1 for op in c["ops"] if op[0] == A)
    n_sdots = int(np.isin(c["a"]["rows"][0], o["touched"]).sum())
    return len(c["ops"]), n_adds, n_sdots, len(o["dots"][1])


TILES = {"m255": 1, "m256": 1, "m257": 2, "m512_full": 2, "ends_at_seam": 2, "straddle_add_remove": 2,
         "straddle_remove_add": 2, "group600": 4, "extremes": 2, "tiles256": 256, "tiles257": 257, "tiles1025": 1025}
OPS = {"m255": 255, "m256": 256, "m257": 257, "m512_full": 512, "extremes": 300, "tiles256": 65_536,
       "tiles257": 65_537, "tiles1025": 262_400}


def test_every_case_is_listed_once():
    assert sorted(M.NAMES) == sorted(list(M.CASES) + list(M.DRAWN)) and len(set(M.NAMES)) == len(M.NAMES)
    assert set(TILES) == set(M.SEAMS) | set(M.DRAWN)


@pytest.mark.parametrize("name", M.NAMES)
def test_case_is_well_formed(name):
    c, o = _case(name)
    a, ops = c["a"], c["ops"]
    rows, (kind, vn, vc) = a["rows"], a["ctx"]
    m = len(ops)
    assert m > 0 and all(0 < op[1] < 1 << 63 for op in ops)
    if name in OPS:
        assert m == OPS[name]
    if name in TILES:
        assert -(-m // M.TILE) == TILES[name]
    # a store: rows ascending by key, {val, ts}, dot; a VV ascending by node
    o5 = np.lexsort((rows[4], rows[3], rows[2], rows[1], rows[0]))
    assert np.array_equal(o5, np.arange(len(o5)))
    assert np.all(vn[1:] > vn[:-1])
    # batch order is not key order, and some add's rank is not its sorted position among the adds
    keys_in_order = [op[1] for op in ops]
    if len(o["touched"]) >= 8:
        assert keys_in_order != sorted(keys_in_order)
        k, _, _, _, rank, _ = M.marshal(ops)
        if k.any():
            assert not np.array_equal(rank[k == 1], np.arange(int(k.sum()), dtype=np.uint64))
    if name not in M.DRAWN and name not in ("all_absent", "long_runs"):
        assert len(a["rows"][0]) == 0 or len(np.unique(a["rows"][0])) >= 3000  # the background
    if name in M.CASES:
        assert np.array_equal(o["touched"], c["keys"])


@pytest.mark.parametrize("name", ["m255", "m256", "m257"])
def test_one_op_per_key(name):
    c, o = _case(name)
    kind, key, _, _, _, _, head, last = _sorted(c)
    assert head.all() and last.all()
    present = np.isin(key, c["a"]["rows"][0])
    for p in (True, False):
        for k in (0, 1):
            assert ((present == p) & (kind == k)).any()
    if name == "m257":  # the one op of the second tile, and the first tile's last
        assert head[255] and head[256] and len(key) == 257


def test_m512_full_ends_a_group_at_the_last_op():
    c, _ = _case("m512_full")
    kind, key, _, _, _, _, head, last = _sorted(c)
    assert len(key) == 2 * M.TILE and head[509] and not head[510] and not head[511] and last[511]
    assert kind[509] == 1 and kind[510] == 0 and kind[511] == 1


def test_ends_at_seam():
    c, _ = _case("ends_at_seam")
    _, key, _, _, _, _, head, last = _sorted(c)
    assert head[253] and not head[254] and not head[255] and last[255]
    assert head[256] and not last[256] and last[257]


@pytest.mark.parametrize("name,first", [("straddle_add_remove", 1), ("straddle_remove_add", 0)])
def test_straddle(name, first):
    c, o = _case(name)
    kind, key, _, _, _, _, head, last = _sorted(c)
    assert head[254] and not head[255:258].any() and last[257] and not last[254:257].any()
    # the last op in the head's tile is not the kind of the group's last op
    assert kind[254] == kind[255] == first and kind[256] == kind[257] == 1 - first
    assert int((c["a"]["rows"][0] == key[254]).sum()) == 2
    assert int((o["delta"][0] == key[254]).sum()) == 1 - first


def test_straddles_share_the_key_and_its_row_appears_once():
    (ca, oa), (cb, ob) = _case("straddle_add_remove"), _case("straddle_remove_add")
    ka, kb = _sorted(ca)[1][254], _sorted(cb)[1][254]
    assert ka == kb
    assert int((oa["delta"][0] == ka).sum()) + int((ob["delta"][0] == kb).sum()) == 1


def test_group600_leaves_a_tile_without_a_head():
    c, o = _case("group600")
    kind, key, _, _, rank, _, head, last = _sorted(c)
    assert len(key) == 800 and head[:101].all() and not head[101:700].any() and head[700:].all()
    assert not head[M.TILE:2 * M.TILE].any()
    assert last[699] and kind[699] == 1 and int(rank[699]) != 599
    assert 0 in kind[100:700].tolist() and int(kind[100:700].sum()) > 300
    assert int((c["a"]["rows"][0] == key[100]).sum()) == 3
    i = np.flatnonzero(o["delta"][0] == key[100])
    assert len(i) == 1 and int(o["delta"][4][i[0]]) == 10 + 1 + int(rank[699])


def test_extremes_lie_on_both_sides_of_the_seam():
    c, o = _case("extremes")
    kind, key, val, ts, _, _, head, _ = _sorted(c)
    assert head.all()
    for at in (250, 256):
        assert kind[at:at + 6].all()
        assert ts[at:at + 4].tolist() == [M.I64_MIN, -1, 0, M.I64_MAX]
        assert val[at + 4:at + 6].tolist() == [0, M.U64_MAX]
        for i in range(at, at + 6):  # ... and reach the delta
            j = np.flatnonzero(o["delta"][0] == key[i])
            assert len(j) == 1 and o["delta"][1][j[0]] == val[i] and o["delta"][2][j[0]] == ts[i]


@pytest.mark.parametrize("name,rounds", [("tiles256", 1), ("tiles257", 2), ("tiles1025", 5)])
def test_scan_rounds(name, rounds):
    c, o = _case(name)
    m, n_adds, n_sdots, n_dots = _counts(c, o)
    tiles = -(-m // M.TILE)
    assert -(-tiles // M.ROUND) == rounds
    assert len(np.unique(c["a"]["rows"][0])) == 20_000
    kind, key, _, _, _, _, head, _ = _sorted(c)
    present = np.isin(key, c["a"]["rows"][0])
    assert present.any() and not present.all() and not head.all() and n_sdots > 0
    if name == "tiles1025":
        assert n_adds >= M.GEN_PASS + 1 and 0 < m - n_adds  # the generator's grid goes round
    else:
        assert 3.5 < n_adds / (m - n_adds) < 4.5
    # every round's tiles count something: the carry into each round is not zero
    per_tile = np.add.reduceat(head.astype(np.int64), np.arange(0, m, M.TILE))
    assert (per_tile > 0).all() and len(set(per_tile.tolist())) > 1
    # the last op opens a group, an add on a present key: the last tile uses all three offsets
    assert head[-1] and kind[-1] == 1 and present[-1]


def test_dot_list_paths():
    """n_sdots == 0, n_adds == 0 and n_dots == 0 where the case's name says so"""
    want = {  # name: (adds?, state dots?)
        "empty_state": (True, False), "all_absent": (True, False), "removes_absent_only": (False, False),
        "removes_only": (False, True)}
    for name, (adds, sdots) in want.items():
        c, o = _case(name)
        m, n_adds, n_sdots, n_dots = _counts(c, o)
        assert (n_adds > 0) == adds and (n_sdots > 0) == sdots, name
        assert n_dots == n_sdots + n_adds and len(o["touched"]) > 0
        kinds = {op[0] for op in c["ops"]}
        assert kinds == ({A, RM} if adds else {RM})
    c, o = _case("empty_state")
    assert len(c["a"]["rows"][0]) == 0 and len(c["a"]["ctx"][1]) == 0
    c, o = _case("removes_absent_only")
    assert len(o["delta"][0]) == 0 and len(o["dots"][1]) == 0
    c, o = _case("removes_only")
    rows = c["a"]["rows"]
    assert all(int((rows[0] == k).sum()) >= 2 for k in o["touched"]) and len(o["delta"][0]) == 0
    c, o = _case("all_absent")
    sk, t = np.unique(c["a"]["rows"][0]), o["touched"]
    assert t[0] < sk[0] and t[-1] > sk[-1]
    between = np.searchsorted(sk, t[1:-1])
    assert ((between > 0) & (between < len(sk))).all() and len(set(between.tolist())) == len(t) - 2


VV_PLACE = {"vv_first": "first", "vv_last": "last", "vv_middle": "middle", "vv_below": "below", "vv_between": "between",
            "vv_above": "above", "vv_single": "single"}


@pytest.mark.parametrize("name", list(VV_PLACE))
def test_the_nodes_place_in_the_vv(name):
    c, o = _case(name)
    _, vn, vc = c["a"]["ctx"]
    node, n = c["node"], len(vn)
    i = int(np.searchsorted(vn, node))
    there = i < n and int(vn[i]) == node
    place = VV_PLACE[name]
    if place == "single":
        assert n == 1 and there and int(vc[0]) > 0
    elif place in ("first", "last", "middle"):
        assert there and n >= 3 and int(vc[i]) > 0
        assert {"first": i == 0, "last": i == n - 1, "middle": 0 < i < n - 1}[place]
    else:
        assert not there and n >= 2
        assert {"below": i == 0, "above": i == n, "between": 0 < i < n}[place]
    # adds, removes, state dots: the sort path, with the node's counter in the generated dots
    m, n_adds, n_sdots, _ = _counts(c, o)
    assert n_adds > 0 and n_sdots > 0 and m > n_adds
    c0 = int(vc[i]) if there else 0
    assert sorted(o["delta"][4].tolist())[0] >= c0 + 1 and int(o["delta"][4].max()) <= c0 + n_adds


def test_vv_counters_differ():
    cs = []
    for name in ("vv_first", "vv_last", "vv_middle", "vv_single"):
        c, _ = _case(name)
        _, vn, vc = c["a"]["ctx"]
        cs.append(int(vc[np.flatnonzero(vn == c["node"])[0]]))
    assert len(set(cs)) == len(cs) and 0 not in cs


def test_wide_dots():
    c, o = _case("wide_dots")
    rows, (_, vn, vc) = c["a"]["rows"], c["a"]["ctx"]
    m, n_adds, n_sdots, n_dots = _counts(c, o)
    sel = np.isin(rows[0], o["touched"])
    nodes, cnts = rows[3][sel], rows[4][sel]
    assert set(M.WIDE_NODES) <= set(nodes.tolist()) and set(M.WIDE_CNTS) <= set(cnts.tolist())
    for x in (1 << 32, 1 << 63):  # (named: the counters a 32-bit or a signed sort gets wrong)
        assert x in cnts.tolist()
    assert c["node"] == M.WIDE_NODE == 65_536 and int(vc[vn == 65_536][0]) == M.WIDE_C == 1 << 40
    c0 = M.WIDE_C + 1  # the first generated counter
    mine = cnts[nodes == 65_536]
    assert (mine < c0).any() and (mine > c0 + n_adds).any() and n_adds > 0
    # the generated dots interleave with the state's in the list, and none collides
    assert n_dots == n_sdots + n_adds
    dn, dc = o["dots"][1], o["dots"][2]
    i = np.flatnonzero((dn == 65_536) & (dc >= c0) & (dc < c0 + n_adds))
    assert len(i) == n_adds and 0 < i[0] and i[-1] < len(dn) - 1
    assert dn[i[0] - 1] == 65_536 and dn[i[-1] + 1] == 65_536
    # a sort over the counters' low 32 bits alone would order the list otherwise
    low = np.lexsort((dc & np.uint64(0xFFFFFFFF), dn))
    assert not np.array_equal(low, np.arange(len(dn)))


def test_long_runs():
    c, o = _case("long_runs")
    rows = c["a"]["rows"]
    first, lastk = rows[0][0], rows[0][-1]
    assert o["touched"].tolist() == [first, lastk]
    assert int((rows[0] == first).sum()) == 1025 and int((rows[0] == lastk).sum()) == 5000
    assert rows[0][-5000] == lastk and rows[0][-5001] != lastk  # the run ends the store
    by_key = {op[1]: op[0] for op in c["ops"]}
    assert by_key == {int(first): A, int(lastk): RM}


def test_many_rows_few_ops_is_past_the_first_capacity():
    c, o = _case("many_rows_few_ops")
    m, n_adds, n_sdots, n_dots = _counts(c, o)
    assert (m, n_adds, n_sdots, n_dots) == (3, 0, 120, 120)
    assert n_dots > 8 * m + n_adds + 1 == 25  # the wrappers' first capacity
    assert n_dots <= len(c["a"]["rows"][0]) + n_adds + 1  # ... and inside the second


def test_own_dot_collides():
    """state rows under touched keys carry dots (node, C[node] + 1 + r), r < n_adds: the oracle's
    set lists each once, so its list is shorter than state dots + adds by the collisions"""
    c, o = _case("own_dot")
    rows, (_, vn, vc) = c["a"]["rows"], c["a"]["ctx"]
    m, n_adds, n_sdots, n_dots = _counts(c, o)
    c0 = int(vc[vn == c["node"]][0])
    sel = np.isin(rows[0], o["touched"])
    hit = sel & (rows[3] == c["node"]) & (rows[4] > c0) & (rows[4] <= c0 + n_adds)
    assert int(hit.sum()) == 3 and n_dots == n_sdots + n_adds - 3
    # each is the row its key's add makes: in both the state and the delta
    srows = set(zip(*[x[hit].tolist() for x in rows]))
    drows = set(zip(*[x.tolist() for x in o["delta"]]))
    assert srows <= drows
