"""The stream kernel's tile loader, commit and stripe counts at the shapes where they can go
wrong (csrc/dg_jtile.h: slot_row, issue_tile, commit_tile; csrc/join_stream.hip:
stripe_load).  Every lane loads a
row for every staging slot, at an index clamped into a store that has rows, and commits it,
so a slot without a row holds a copy of a real one that the merge must not use.  The shapes
are those where slots have no row or a store has none: an empty side (null columns), one
row, tiles that hold rows of one side only, a last tile of one position, and totals at the
tile and the fused / partitioned boundaries.  Engines of one and two workgroups (DG_JOIN_WORKERS) make one workgroup run
iterations 1-3 of the loop, whose prefetch a small join on the default engine never
reaches: at most FUSE_IT tiles per workgroup run the fused kernel, more the partitioned one;
DG_JOIN_MODE=2 (slot + compact kernels, the same loader) is the control.  Bit-exact against
the C oracle (rows, context, changed keys), dg_store_check on every output."""
import functools

import numpy as np
import pytest

import join_routes as J
from oracle import ref as R
from test_gpu_join_variants import _engine, check_call
from test_gpu_parity import up

pytestmark = pytest.mark.gpu

JT = J.JOIN_TILE
ENGINES = {"w1": {"DG_JOIN_WORKERS": "1"}, "w2": {"DG_JOIN_WORKERS": "2"}, "twopass": {"DG_JOIN_MODE": "2"}}
# two version vectors with node ids below VT (FAST; fused: the merge without the coverage
# search), with ids of VT and above (FAST, the searching merge), and two dot sets
BASES = ("near", "far_both", "dots_dots")


@pytest.fixture(scope="module")
def engines():
    made = {name: _engine(env) for name, env in ENGINES.items()}
    yield made
    for e in made.values():
        e.close()


def _sel(rep, idx):
    return {"rows": tuple(np.ascontiguousarray(c[idx]) for c in rep["rows"]), "ctx": rep["ctx"]}


def _with(rep, i, col, value):
    """Row i of `rep` alone, column `col` set to `value`."""
    rows = [np.ascontiguousarray(c[i:i + 1]).copy() for c in rep["rows"]]
    if col is not None:
        rows[col][0] = value
    return {"rows": tuple(rows), "ctx": rep["ctx"]}


def _prefix_pair(a, b, total):
    """Prefixes of a and b of `total` rows together, in the stores' proportion."""
    na_all, nb_all = len(a["rows"][0]), len(b["rows"][0])
    assert na_all + nb_all >= total
    na = total * na_all // (na_all + nb_all)
    return _sel(a, slice(0, na)), _sel(b, slice(0, total - na))


@functools.lru_cache(maxsize=None)
def shapes(base):
    """label -> (x, y), each joined in both orders."""
    a, b = J.layout(base)
    ka, kb = a["rows"][0], b["rows"][0]
    na, nb = len(ka), len(kb)
    assert na > 6000 and nb > 6000
    none = slice(0, 0)
    out = {}
    # an empty side: against one row, three tiles on one workgroup, six (the partitioned
    # kernel on one workgroup, three fused iterations on two)
    for n in (1, 2500, 5200):
        out["empty_%d" % n] = (_sel(a, none), _sel(b, slice(0, n)))
    # one row each: the same row (equal dot), its key with another value, another key
    r = 17
    out["one_same"] = (_with(a, r, None, 0), {"rows": _with(a, r, None, 0)["rows"], "ctx": b["ctx"]})
    out["one_value"] = (_with(a, r, None, 0), {"rows": _with(a, r, 1, a["rows"][1][r] ^ np.uint64(5))["rows"],
                                               "ctx": b["ctx"]})
    other = int(np.flatnonzero(kb != ka[r])[0])
    out["one_key"] = (_with(a, r, None, 0), _with(b, other, None, 0))
    # disjoint key ranges: tiles of one side only and one tile across the seam
    for n in (2000, 2600):
        lo = _sel(a, slice(0, n))
        above = np.flatnonzero(kb > ka[n - 1])[:n]
        assert len(above) == n
        out["disjoint_a_below_%d" % n] = (lo, _sel(b, above))
        hi = _sel(a, slice(na - n, na))
        below = np.flatnonzero(kb < ka[na - n])[-n:]
        assert len(below) == n
        out["disjoint_a_above_%d" % n] = (hi, _sel(b, below))
    # skew: one row of b against n rows of a, in the first, a middle and the last tile
    for n in (4000, 4100):
        j = nb // 2
        up_, down = np.flatnonzero(ka > kb[j]), np.flatnonzero(ka < kb[j])
        assert len(up_) >= n and len(down) >= n
        one = _sel(b, slice(j, j + 1))
        out["skew_first_%d" % n] = (one, _sel(a, up_[:n]))
        out["skew_last_%d" % n] = (one, _sel(a, down[-n:]))
        out["skew_middle_%d" % n] = (one, _sel(a, np.concatenate([down[-(n // 2):], up_[:n - n // 2]])))
    # totals around the tile boundaries: a last tile of one position, and on one workgroup
    # the largest fused launch and the smallest partitioned one
    for total in (JT - 1, JT, JT + 1, J.FUSE_IT * JT, J.FUSE_IT * JT + 1):
        out["total_%d" % total] = _prefix_pair(a, b, total)
    return out


# (the labels of shapes(), spelled out so that collection builds no input)
LABELS = ["empty_1", "empty_2500", "empty_5200", "one_same", "one_value", "one_key",
          "disjoint_a_below_2000", "disjoint_a_above_2000", "disjoint_a_below_2600", "disjoint_a_above_2600",
          "skew_first_4000", "skew_last_4000", "skew_middle_4000", "skew_first_4100", "skew_last_4100",
          "skew_middle_4100"] + ["total_%d" % t for t in (JT - 1, JT, JT + 1, J.FUSE_IT * JT, J.FUSE_IT * JT + 1)]


def _pair(base, label, order):
    x, y = shapes(base)[label]
    return (x, y) if order == "xy" else (y, x)


@functools.lru_cache(maxsize=None)
def expected(base, label, order, keyed):
    """The oracle's (rows, context, changed keys) of a call, computed once for all engines."""
    x, y = _pair(base, label, order)
    ks = keyset(base, label) if keyed else None
    rows, ctx = R.join2(x["rows"], x["ctx"], y["rows"], y["ctx"], keys=ks)
    return rows, ctx, R.changed_keys(x["rows"], rows, ks)


def keyset(base, label):
    x, y = shapes(base)[label]
    return J.union_keys(x, y)[::2]


def run(engines, on, base, label, chg=False, keyed=False, routes=None):
    for order in ("xy", "yx"):
        x, y = _pair(base, label, order)
        ks = keyset(base, label) if keyed else None
        nx, ny = len(x["rows"][0]), len(y["rows"][0])
        if keyed:
            assert not J.splice_wanted(nx, ny, len(ks))
        workers, two_pass = int(ENGINES[on].get("DG_JOIN_WORKERS", 0)), "DG_JOIN_MODE" in ENGINES[on]
        r = J.route(nx, ny, workers=max(workers, 1), two_pass=two_pass, chg=chg, keyed=keyed,
                    kind_a=x["ctx"][0], kind_b=y["ctx"][0])
        what = (on, base, label, order, r["route"], "changes" if chg else "join2", "keyed" if keyed else "all")
        if routes is not None:
            assert r["route"] == routes, what
        check_call(engines[on], up(x) + up(y), ks, chg, expected(base, label, order, keyed), what)


def test_shapes_are_what_they_say():
    """The tile counts the cases rely on (the model of tests/join_routes.py): on one
    workgroup 2,500 rows are three fused tiles, 5,200 rows the partitioned kernel, and
    FUSE_IT * JT / FUSE_IT * JT + 1 rows the two sides of the boundary, the last tile of the
    latter one position."""
    r = J.route(0, 2500, workers=1)
    assert (r["route"], r["ntiles"], r["stripes"]) == ("fused", 3, 3) and r["jt"] <= JT
    assert J.route(0, 5200, workers=1)["route"] == "partitioned"
    assert J.route(0, 5200, workers=2)["route"] == "fused" and J.route(0, 5200, workers=2)["stripes"] == 3
    r = J.route(J.FUSE_IT * JT, 0, workers=1)
    assert (r["route"], r["stripes"]) == ("fused", J.FUSE_IT)
    r = J.route(J.FUSE_IT * JT, 1, workers=1)
    assert (r["route"], r["ntiles"], r["jt"]) == ("partitioned", J.FUSE_IT + 1, JT)
    assert J.route(JT, 1, workers=1)["ntiles"] == 2
    for n in (4000, 4100):
        assert J.route(1, n, workers=1)["route"] == ("fused" if n == 4000 else "partitioned")
    assert set(LABELS) == set(shapes("near"))


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("on", ("w1", "w2"))
def test_two_version_vectors(engines, on, label):
    """FAST: every shape on one and on two workgroups, node ids below VT."""
    run(engines, on, "near", label)


@pytest.mark.parametrize("label", LABELS)
def test_far_version_vectors(engines, label):
    """FAST with node ids of VT and above (the merge that searches the VVs in global memory,
    whose flat loads share the tile loads' counter), one workgroup."""
    run(engines, "w1", "far_both", label)


@pytest.mark.parametrize("label", LABELS)
def test_dot_sets(engines, label):
    """Every shape once with dot-set contexts, one workgroup."""
    run(engines, "w1", "dots_dots", label)


@pytest.mark.parametrize("label", LABELS)
def test_two_pass_control(engines, label):
    """DG_JOIN_MODE=2: the slot and compact kernels on the same shapes."""
    run(engines, "twopass", "near", label, routes="two_pass")


@pytest.mark.parametrize("on", ("w1", "w2"))
@pytest.mark.parametrize("label", ("empty_2500", "empty_5200", "disjoint_a_below_2600", "skew_middle_4100",
                                   "total_%d" % (J.FUSE_IT * JT + 1)))
def test_keyed(engines, on, label):
    """KEYED: every second key of the union (the keyset slice loads ride behind the tile's)."""
    run(engines, on, "near", label, keyed=True)


@pytest.mark.parametrize("on", ("w1", "w2"))
@pytest.mark.parametrize("label", ("empty_2500", "disjoint_a_above_2600", "skew_last_4100", "one_value",
                                   "total_%d" % (J.FUSE_IT * JT), "total_%d" % (J.FUSE_IT * JT + 1)))
def test_changes(engines, on, label):
    """CHG: dg_join2_changes, unkeyed and keyed."""
    run(engines, on, "near", label, chg=True)
    run(engines, on, "near", label, chg=True, keyed=True)
