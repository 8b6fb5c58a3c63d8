"""The CPU model of launch_join2's choice of kernels (tests/join_routes.py): pinned to the
constants and the decisions of csrc/dg_launch.h, the join's units and csrc/api_join.hip, and
-- for every (engine, shape) pair tests/test_gpu_join_variants.py joins -- the model's
answer pinned here, so a retune of the tile, of FUSE_IT or of the grid's bound fails a test
instead of silently moving the GPU cases off the kernels they are for.  Also the
conditions those cases rely on, checked on the C oracle's results."""
import os
import re

import numpy as np
import pytest

import join_routes as J
from oracle import ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "delta_crdt_ex_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# the join's kernels and launchers: launch_join2 and the partition (join.hip), the stream
# kernel, the two-pass pair, and the two headers they share
JOIN_UNITS = ("join.hip", "join_stream.hip", "join_twopass.hip", "dg_jtile.h", "dg_jsplit.h")


# ---------------------------------------------------------------- the model is the sources'

def test_constants_match_the_sources():
    """join_routes.CONST restates csrc/dg_launch.h and the join's units (JOIN_UNITS): if the
    tile, FUSE_IT, VT, KS or the grid's bound moves there, the model is wrong until it
    follows."""
    h, j, api = _src("dg_launch.h"), "\n".join(_src(u) for u in JOIN_UNITS), _src("api_join.hip")
    got = {}
    for name in ("DG_JOIN_BLOCK", "DG_JOIN_ITEMS"):
        got[name] = int(re.search(r"#define\s+%s\s+(\d+)" % name, h).group(1))
    got["JOIN_TILE_LESS"] = int(re.search(
        r"constexpr\s+int\s+JOIN_TILE\s*=\s*JOIN_BLOCK\s*\*\s*JOIN_ITEMS\s*-\s*(\d+)\s*;", h).group(1))
    for name in ("FUSE_IT", "VT", "KS"):
        got[name] = int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, j).group(1))
    got["CQ_SPAN"] = int(re.search(r"constexpr\s+int\s+CQ\s*=\s*\((\d+)\s*\+\s*JB\s*-\s*1\)\s*/\s*JB\s*;", j).group(1))
    got["SPLICE_FACTOR"] = int(re.search(r"\(n_keys \+ b->n\) \* (\d+) <= a->n", api).group(1))
    assert got == J.CONST, "the join's constants moved: tests/join_routes.py's model must follow them"
    assert re.search(r"JOIN_BLOCK\s*=\s*DG_JOIN_BLOCK\s*;", h) and re.search(r"JOIN_ITEMS\s*=\s*DG_JOIN_ITEMS\s*;", h)
    assert re.search(r"constexpr\s+int\s+JB\s*=\s*JOIN_BLOCK\s*;", j) and re.search(r"constexpr\s+int\s+JT\s*=\s*JOIN_TILE\s*;", j)
    assert (J.JOIN_TILE, J.CQ) == (1016, 2)
    # the decisions, as the model restates them
    for line in ("return (na + nb + JOIN_TILE - 1) / JOIN_TILE;",):
        assert line in h
    for line in ("const bool fast = ca.kind == 0 && cb.kind == 0;",
                 "const bool stream = mode != JOIN_TWO_PASS || chg_tmp;",
                 "g = workers > 0 ? (u64)workers : resident_grid((const void*)kern);",
                 "g = std::min<u64>(std::min<u64>(p.ntiles, g), (u64)CQ * JB);",
                 "const u64 gr = workers > 0 ? g + 1 : resident_grid((const void*)kern_late);",
                 "const u64 gt = std::min<u64>(std::min<u64>(p.ntiles, gr - 1), (u64)CQ * JB);",
                 "if (!no_fuse && gr >= 2 && p.ntiles <= (u64)FUSE_IT * gt) {",
                 "if (!chg_tmp) balance_tiles(p, gt);",
                 "if (G == 0 || p.ntiles <= G) return;",
                 "const u64 k = (p.ntiles + G - 1) / G;",
                 "const u64 jt = std::min<u64>(((total + k * G - 1) / (k * G) + 1) & ~1ull, JT);",
                 "p.ntiles = (total + jt - 1) / jt;",
                 "if (LATE && FAST && !vv_far)",
                 "far |= nd >= (u32)VT;",
                 "hipLaunchKernelGGL(kern, dim3((unsigned)p.ntiles), dim3(JB), 0, st, p);"):
        assert line in j, line
    assert "(force_two_pass || e->join_mode == JOIN_TWO_PASS) && !chg" in api
    e = _src("api_engine.hip")
    assert 'getenv("DG_JOIN_WORKERS")' in e and 'getenv("DG_JOIN_MODE")' in e and "m[0] == '2'" in e


def test_engine_params():
    assert {n: J.engine_params(n) for n in J.ENGINES} == {
        "default": (0, False), "fused4": (6, False), "part2": (2, False), "part1": (1, False),
        "twopass": (0, True)}


def test_route_model_by_hand():
    """The model on figures worked out from launch_join2 by hand."""
    JT = J.JOIN_TILE
    # one workgroup per tile by default, whatever the size (inside the model's range)
    r = J.route(30 * JT, 0)
    assert (r["route"], r["G"], r["stripes"], r["jt"]) == ("fused", 30, 1, JT)
    with pytest.raises(AssertionError):
        J.route((J.DEFAULT_MAX_TILES + 1) * JT, 0)
    # 6 workers: fused up to 24 tiles; 21 tiles re-cut to 24 even tiles, not when chg
    r = J.route(10000, 10326, workers=6)
    assert (r["route"], r["G"], r["jt"], r["ntiles"], r["stripes"], r["last"]) == ("fused", 6, 848, 24, 4, 6)
    r = J.route(10000, 10326, workers=6, chg=True)
    assert (r["route"], r["G"], r["jt"], r["ntiles"], r["stripes"], r["last"]) == ("fused", 6, JT, 21, 4, 3)
    assert J.route(24 * JT, 0, workers=6)["route"] == "fused"
    assert J.route(24 * JT, 1, workers=6)["route"] == "partitioned"
    # a grid larger than the tiles is cut to them; and to CQ * JB workgroups
    assert J.route(3 * JT, 0, workers=1024)["G"] == 3
    r = J.route(5000 * JT, 0, workers=2048)
    assert (r["route"], r["G"]) == ("partitioned", 1024)
    assert J.route(4096 * JT, 0, workers=2048)["route"] == "fused"
    # two-pass: one workgroup per tile; the changes call stays single-pass
    r = J.route(10000, 10326, two_pass=True)
    assert (r["route"], r["G"], r["kernel"]) == ("two_pass", 21, ("slot", True, False))
    assert J.route(10000, 10326, two_pass=True, chg=True)["route"] == "fused"
    assert J.route(0, 0, workers=2)["route"] == "empty"
    # the merge body: nofb only on the fused kernel with every VV node id below VT
    vt = J.VT
    assert J.route(100, 100, vv_a=(0, vt - 1), vv_b=(3,))["merge"] == "nofb"
    assert J.route(100, 100, vv_a=(0, vt), vv_b=(3,))["merge"] == "search"
    assert J.route(100, 100, vv_a=(0,), vv_b=(2 ** 32 - 1,))["merge"] == "search"
    assert J.route(100 * JT, 100, workers=2, vv_a=(0,), vv_b=(1,))["merge"] == "search"
    assert J.route(100, 100, two_pass=True, vv_a=(0,), vv_b=(1,))["merge"] == "search"
    assert J.route(100, 100, kind_a=J.DOTS)["merge"] == "dots"
    assert J.route(100, 100, kind_b=J.DOTS, keyed=True, chg=True)["kernel"] == (False, True, True, True)
    # the splice takes a keyed join when (|K| + |B|) * 8 <= |A|
    assert J.splice_wanted(800, 50, 50) and not J.splice_wanted(799, 50, 50)
    assert not J.splice_wanted(800, 0, 0)


def test_key_slices_by_hand():
    """Tile t's slice is [ksplit(t), min(ksplit(t + 1) + 1, |K|)): the keys of merged
    positions t * jt and (t + 1) * jt bound it, the second inclusively."""
    ka = np.array([10, 20, 30, 40], np.uint64)
    kb = np.array([15, 20, 50, 60], np.uint64)   # merged: 10 15 20 20 30 40 50 60
    keys = np.array([5, 20, 30, 55, 70], np.uint64)
    # jt = 4: boundaries at merged keys 10, 30, (end) -> ksplit 1, 2, 5
    assert J.key_slices(ka, kb, keys, 4).tolist() == [2, 3]
    # jt = 3: boundaries 10, 20, 50, (end) -> ksplit 1, 1, 3, 5
    assert J.key_slices(ka, kb, keys, 3).tolist() == [1, 3, 2]


# ---------------------------------------------------------------- the GPU file's shapes

# (rows in, shapes): engine -> "dg_join2 | dg_join2_changes", each
# "route G jt ntiles stripes last".  The five VV layouts of the sparse base pair hold the
# same rows but for their node ids, and likewise the others.
PINS = {
    (20486, ('near', 'far_both', 'far_rows_only', 'far_a_only', 'far_b_only')): {
        'default': 'fused 21 1016 21 1 21 | fused 21 1016 21 1 21',
        'fused4': 'fused 6 854 24 4 6 | fused 6 1016 21 4 3',
        'part2': 'partitioned 2 1016 21 11 1 | partitioned 2 1016 21 11 1',
        'part1': 'partitioned 1 1016 21 21 1 | partitioned 1 1016 21 21 1',
        'twopass': 'two_pass 21 1016 21 1 21 | fused 21 1016 21 1 21',
    },
    (20485, ('dense_near', 'dense_far_both')): {
        'default': 'fused 21 1016 21 1 21 | fused 21 1016 21 1 21',
        'fused4': 'fused 6 854 24 4 6 | fused 6 1016 21 4 3',
        'part2': 'partitioned 2 1016 21 11 1 | partitioned 2 1016 21 11 1',
        'part1': 'partitioned 1 1016 21 21 1 | partitioned 1 1016 21 21 1',
        'twopass': 'two_pass 21 1016 21 1 21 | fused 21 1016 21 1 21',
    },
    (20307, ('dots_dots', 'vv_dots', 'dots_vv')): {
        'default': 'fused 20 1016 20 1 20 | fused 20 1016 20 1 20',
        'fused4': 'fused 6 848 24 4 6 | fused 6 1016 20 4 2',
        'part2': 'partitioned 2 1016 20 10 2 | partitioned 2 1016 20 10 2',
        'part1': 'partitioned 1 1016 20 20 1 | partitioned 1 1016 20 20 1',
        'twopass': 'two_pass 20 1016 20 1 20 | fused 20 1016 20 1 20',
    },
    (12055, ('a_empty',)): {
        'default': 'fused 12 1016 12 1 12 | fused 12 1016 12 1 12',
        'fused4': 'fused 6 1006 12 2 6 | fused 6 1016 12 2 6',
        'part2': 'partitioned 2 1016 12 6 2 | partitioned 2 1016 12 6 2',
        'part1': 'partitioned 1 1016 12 12 1 | partitioned 1 1016 12 12 1',
        'twopass': 'two_pass 12 1016 12 1 12 | fused 12 1016 12 1 12',
    },
    (8431, ('b_empty',)): {
        'default': 'fused 9 1016 9 1 9 | fused 9 1016 9 1 9',
        'fused4': 'fused 6 704 12 2 6 | fused 6 1016 9 2 3',
        'part2': 'partitioned 2 1016 9 5 1 | partitioned 2 1016 9 5 1',
        'part1': 'partitioned 1 1016 9 9 1 | partitioned 1 1016 9 9 1',
        'twopass': 'two_pass 9 1016 9 1 9 | fused 9 1016 9 1 9',
    },
    (0, ('both_empty',)): {
        'default': 'empty 0 1016 0 0 0 | empty 0 1016 0 0 0',
        'fused4': 'empty 0 1016 0 0 0 | empty 0 1016 0 0 0',
        'part2': 'empty 0 1016 0 0 0 | empty 0 1016 0 0 0',
        'part1': 'empty 0 1016 0 0 0 | empty 0 1016 0 0 0',
        'twopass': 'empty 0 1016 0 0 0 | empty 0 1016 0 0 0',
    },
    (2, ('one_row_each',)): {
        'default': 'fused 1 1016 1 1 1 | fused 1 1016 1 1 1',
        'fused4': 'fused 1 1016 1 1 1 | fused 1 1016 1 1 1',
        'part2': 'fused 1 1016 1 1 1 | fused 1 1016 1 1 1',
        'part1': 'fused 1 1016 1 1 1 | fused 1 1016 1 1 1',
        'twopass': 'two_pass 1 1016 1 1 1 | fused 1 1016 1 1 1',
    },
    (24384, ('boundary_fused4_0',)): {
        'default': 'fused 24 1016 24 1 24 | fused 24 1016 24 1 24',
        'fused4': 'fused 6 1016 24 4 6 | fused 6 1016 24 4 6',
        'part2': 'partitioned 2 1016 24 12 2 | partitioned 2 1016 24 12 2',
        'part1': 'partitioned 1 1016 24 24 1 | partitioned 1 1016 24 24 1',
        'twopass': 'two_pass 24 1016 24 1 24 | fused 24 1016 24 1 24',
    },
    (24385, ('boundary_fused4_1',)): {
        'default': 'fused 25 1016 25 1 25 | fused 25 1016 25 1 25',
        'fused4': 'partitioned 6 1016 25 5 1 | partitioned 6 1016 25 5 1',
        'part2': 'partitioned 2 1016 25 13 1 | partitioned 2 1016 25 13 1',
        'part1': 'partitioned 1 1016 25 25 1 | partitioned 1 1016 25 25 1',
        'twopass': 'two_pass 25 1016 25 1 25 | fused 25 1016 25 1 25',
    },
    (8128, ('boundary_part2_0',)): {
        'default': 'fused 8 1016 8 1 8 | fused 8 1016 8 1 8',
        'fused4': 'fused 6 678 12 2 6 | fused 6 1016 8 2 2',
        'part2': 'fused 2 1016 8 4 2 | fused 2 1016 8 4 2',
        'part1': 'partitioned 1 1016 8 8 1 | partitioned 1 1016 8 8 1',
        'twopass': 'two_pass 8 1016 8 1 8 | fused 8 1016 8 1 8',
    },
    (8129, ('boundary_part2_1',)): {
        'default': 'fused 9 1016 9 1 9 | fused 9 1016 9 1 9',
        'fused4': 'fused 6 678 12 2 6 | fused 6 1016 9 2 3',
        'part2': 'partitioned 2 1016 9 5 1 | partitioned 2 1016 9 5 1',
        'part1': 'partitioned 1 1016 9 9 1 | partitioned 1 1016 9 9 1',
        'twopass': 'two_pass 9 1016 9 1 9 | fused 9 1016 9 1 9',
    },
}
PIN_OF = {label: (total, row) for (total, labels), row in PINS.items() for label in labels}


def _cell(r):
    return "%s %d %d %d %d %d" % (r["route"], r["G"], r["jt"], r["ntiles"], r["stripes"], r["last"])


def test_every_gpu_shape_is_pinned():
    """Every shape of the GPU file, both orders, on every engine: rows in, route, grid, tile
    size, tiles, stripes and the last stripe's tiles as pinned; the merge body and the
    kernel's template arguments as the layout's table says."""
    shapes = J.shapes()
    assert sorted(s[0] for s in shapes) == sorted(PIN_OF)
    for label, a, b in shapes:
        total, row = PIN_OF[label]
        assert len(a["rows"][0]) + len(b["rows"][0]) == total, label
        for x, y in ((a, b), (b, a)):
            for eng in J.ENGINES:
                got = " | ".join(_cell(J.route_of(eng, x, y, chg=chg)) for chg in (False, True))
                assert got == row[eng], (label, eng)
                for chg in (False, True):
                    for keys in (None, True):
                        r = J.route_of(eng, x, y, chg=chg, keys=keys)
                        if r["route"] == "empty":
                            continue
                        fast = x["ctx"][0] == J.VV and y["ctx"][0] == J.VV
                        want = (("slot", fast, keys is not None) if r["route"] == "two_pass" else
                                (fast, keys is not None, chg, r["route"] == "fused"))
                        assert r["kernel"] == want and r["fast"] == fast
                        if label in J.LAYOUTS:
                            assert r["merge"] == J.MERGE[label][r["route"] != "fused"], (label, eng)


@pytest.mark.parametrize("engine", list(J.ENGINES))
def test_intended_routes(engine):
    """What each engine is for, at the layouts' 20 or 21 tiles: `default` one tile per
    workgroup; `fused4` four fused iterations -- every stripe full after the re-cut, the
    last one part empty when the changes call keeps JT; `part2` / `part1` the partitioned
    kernel on ten or more stripes; `twopass` the slot and compact kernels, and the single
    pass for the changes call."""
    for name in J.LAYOUTS:
        a, b = J.layout(name)
        for chg in (False, True):
            r = J.route_of(engine, a, b, chg=chg)
            assert r["route"] == J.ENGINES[engine][1][chg]
            if engine == "default" or (engine == "twopass" and chg):
                assert r["stripes"] == 1 and r["G"] == r["ntiles"]
            elif engine == "fused4":
                assert r["stripes"] == J.FUSE_IT and r["G"] == 6
                assert (r["last"] < r["G"] and r["jt"] == J.JOIN_TILE) if chg else \
                    (r["last"] == r["G"] and r["jt"] < J.JOIN_TILE and r["ntiles"] == 24)
            elif engine in ("part2", "part1"):
                assert r["stripes"] >= 10 and r["G"] == J.engine_params(engine)[0]
    for e in J.BOUNDARY_ENGINES:
        G = J.engine_params(e)[0]
        r0, r1 = (J.route_of(e, *J.boundary(e, over)) for over in (0, 1))
        assert (r0["route"], r0["ntiles"], r0["jt"]) == ("fused", J.FUSE_IT * G, J.JOIN_TILE)
        assert (r1["route"], r1["ntiles"], r1["last"]) == ("partitioned", J.FUSE_IT * G + 1, 1)


# ---------------------------------------------------------------- the inputs

@pytest.mark.parametrize("name", list(J.LAYOUTS))
def test_layout_inputs(name):
    """A layout's stores are stores (sorted, unique), its contexts sorted; node ids and
    contexts as its name says; the oracle's results meet the conditions the GPU tests rely
    on (join_routes.input_conditions); and the keysets fall on the two sides of KS."""
    a, b = J.layout(name)
    base, table, drop, to_vv = J.LAYOUTS[name]
    for side, rep in zip("ab", (a, b)):
        assert R.store_check(rep["rows"])
        kind, node, cnt = rep["ctx"]
        o = np.lexsort((cnt, node))
        assert np.array_equal(o, np.arange(len(node)))
        nodes = set(np.unique(rep["rows"][3]).tolist())
        assert nodes == set(table.tolist()) | {J.LOW_ABSENT, J.FAR_ABSENT, 1000}
        if base != "dots" or side in to_vv:
            assert kind == J.VV and len(np.unique(node)) == len(node)
            want = [n for n in table.tolist() if not (side in drop and n >= J.VT)]
            assert node.tolist() == want
        else:
            assert kind == J.DOTS and set(node.tolist()) == set(table.tolist())
    fig = J.input_conditions(name)
    if name == "far_both":  # (the figures of the sparse pair, with the hand-made rows)
        assert fig[("ab", None)][:3] == (8431, 12055, 10106) and fig[("ab", "far")] == (11320, 5999)
    if name == "far_rows_only":
        assert fig[("ab", None)][2] == 15395 and fig[("ab", "far")] == (11320, 11288)
    ks = J.keysets(a, b)
    keys = J.union_keys(a, b)
    assert 0 in ks["sparse"] and J.TOP in ks["sparse"] and not np.isin(ks["half"], keys, invert=True).any()
    assert int(np.isin(ks["sparse"], keys, invert=True).sum()) >= 40
    for jt in {J.route_of(e, a, b)["jt"] for e in J.ENGINES}:
        half = J.key_slices(a["rows"][0], b["rows"][0], ks["half"], jt)
        sparse = J.key_slices(a["rows"][0], b["rows"][0], ks["sparse"], jt)
        assert np.median(half) > J.KS and int((half > J.KS).sum()) >= len(half) - 1   # global search
        assert 0 < sparse.max() <= J.KS                                               # the LDS slice


def test_edge_and_boundary_inputs():
    for label, a, b in J.shapes():
        if label in J.LAYOUTS:
            continue
        assert R.store_check(a["rows"]) and R.store_check(b["rows"]), label
        assert a["ctx"][0] == J.VV and a["ctx"][1].tolist() == J.FAR.tolist() == b["ctx"][1].tolist()
    e = J.edges()
    assert [len(r["rows"][0]) for r in e["both_empty"]] == [0, 0]
    assert [len(r["rows"][0]) for r in e["one_row_each"]] == [1, 1]
    assert len(e["a_empty"][0]["rows"][0]) == 0 and len(e["b_empty"][1]["rows"][0]) == 0
