"""The join kernels no other test selects (csrc/join.hip, join_stream.hip,
join_twopass.hip): node ids of VT = 64 and above in
rows and version vectors -- the fused kernel's two merge bodies and the searching coverage
of the partitioned and two-pass kernels -- and small grids: four fused iterations per
workgroup, the partitioned stream kernel on one and two workgroups, and the two-pass
kernels, each with keysets, change events, dot-set and mixed contexts at about 20,000
merged rows.  Engines with DG_JOIN_WORKERS / DG_JOIN_MODE set select the kernels;
tests/join_routes.py models launch_join2's choice, and every call asserts through it that
it lands on the kernel and merge body it is for.  Bit-exact against the C oracle (R.join2,
R.changed_keys), dg_store_check on every output."""
import os

import numpy as np
import pytest

import join_routes as J
from delta_crdt_ex_amd.store import Engine, u64
from oracle import ref as R
from test_gpu_join_delta import kdev
from test_gpu_parity import up

pytestmark = pytest.mark.gpu


def _engine(env):
    """An engine whose dg_engine_create reads `env` (the variables are read there)."""
    os.environ.update(env)
    try:
        return Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def engines(engine):
    made = {name: _engine(env) for name, (env, _) in J.ENGINES.items() if env}
    yield dict(made, default=engine)
    for e in made.values():
        e.close()


def _same(what, got, want):
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, "first difference at", i, got[i], want[i]))


def check_call(eng, dev, ks, chg, want, what):
    """One dg_join2 / dg_join2_changes call of the uploaded pair `dev` against the oracle's
    (rows, context, changed)."""
    sx, cx, sy, cy = dev
    kt = None if ks is None else kdev(ks)
    if chg:
        out, octx, changed = eng.join2_changes(sx, cx, sy, cy, keys=kt)
    else:
        out, octx = eng.join2(sx, cx, sy, cy, keys=kt)
    wr, wc, wch = want
    assert out.n == len(wr[0]), (what, "rows", out.n, len(wr[0]))
    for name, g, w in zip(("key", "val", "ts", "node", "cnt"), out.to_numpy(), wr):
        _same(what + (name,), g, w)
    assert octx.kind == wc[0], what
    node, cnt = octx.to_numpy()
    _same(what + ("ctx node",), node, wc[1])
    _same(what + ("ctx cnt",), cnt, wc[2])
    if chg:
        _same(what + ("changed",), u64(changed), wch)
    if out.n:
        eng.store_check(out)


def check_pair(engines, engine, x, y, want_of, routes, merge=None, keysets=J.KEYSETS, ks_of=None):
    """join(x, y) unkeyed and with each keyset, dg_join2 and dg_join2_changes: first that
    the model sends the call where `routes` = (dg_join2, dg_join2_changes) and `merge`
    say, and that a keyed call is not the splice's; then the call."""
    nx, ny = len(x["rows"][0]), len(y["rows"][0])
    dev = up(x) + up(y)
    for ks_name in keysets:
        ks = None if ks_name is None else ks_of(ks_name)
        if ks is not None:
            assert (len(ks) + ny) * 8 > nx and not J.splice_wanted(nx, ny, len(ks))
        want = want_of(ks_name, ks)
        for chg in (False, True):
            r = J.route_of(engine, x, y, chg=chg, keys=ks)
            what = (engine, r["route"], r["merge"], ks_name, "changes" if chg else "join2")
            assert r["route"] == routes[chg], what
            if merge is not None:
                assert r["merge"] == merge[r["route"] != "fused"], what
            check_call(engines[engine], dev, ks, chg, want, what)


# part1: a few cases only (the route of part2 on one workgroup: every stripe one tile)
CASES = [(e, n) for e in ("default", "fused4", "part2", "twopass") for n in J.LAYOUTS] + \
        [("part1", n) for n in ("far_both", "far_b_only", "dots_vv")]


@pytest.mark.parametrize("on,name", CASES)
def test_layout(engines, on, name):
    """A layout on an engine, both orders, unkeyed, with every second key of the union
    (the keyset searched in global memory) and with every 40th key plus absent ones (the
    LDS slice), dg_join2 and dg_join2_changes.  The layouts: node ids below VT (the
    control), ids of VT and above in rows and both VVs, in the rows alone (the fused
    kernel's `cov = dc == 0`; elsewhere a search that finds nothing), in one side's VV
    alone (vv_far raised by one loop of fill_vv_tables; one direction of coverage finds
    entries, the other none), dense VVs, and dot-set and mixed contexts; every one with
    hand-made counter-0 rows on a node no context names, below VT and above it."""
    J.input_conditions(name)
    a, b = J.layout(name)
    for order, (x, y) in (("ab", (a, b)), ("ba", (b, a))):
        check_pair(engines, on, x, y, lambda ks_name, ks: J.expected(name, order, ks_name),
                   J.ENGINES[on][1], J.MERGE[name], ks_of=lambda n: J.keyset(a, b, n))


def _oracle(x, y):
    def want(ks_name, ks):
        rows, ctx = R.join2(x["rows"], x["ctx"], y["rows"], y["ctx"], keys=ks)
        return rows, ctx, R.changed_keys(x["rows"], rows, ks)
    return want


@pytest.mark.parametrize("on", list(J.ENGINES))
def test_edges(engines, on):
    """a empty, b empty, both empty (the context union alone) and one row each, with far
    VVs: unkeyed and with every second key."""
    for label, (a, b) in J.edges().items():
        for x, y in ((a, b), (b, a)):
            keys = J.union_keys(x, y)
            r = [J.route_of(on, x, y, chg=chg)["route"] for chg in (False, True)]
            if label == "both_empty":
                assert r == ["empty", "empty"]
            elif label == "one_row_each":
                assert r == ["two_pass" if on == "twopass" else "fused", "fused"]
            check_pair(engines, on, x, y, _oracle(x, y), r,
                       keysets=(None, "half") if len(keys) else (None,), ks_of=lambda n: keys[::2])


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("on", J.BOUNDARY_ENGINES)
def test_fused_partitioned_boundary(engines, on, over):
    """Exactly FUSE_IT * G tiles, every one full (the largest fused launch: each workgroup
    searches the splits of all FUSE_IT tiles), and one row more (the partitioned launch on
    FUSE_IT + 1 stripes, the last tile a single row)."""
    a, b = J.boundary(on, over)
    keys = J.union_keys(a, b)
    sets = {"half": keys[::2], "sparse": np.union1d(keys[5::40], np.array([0, J.TOP], np.uint64))}
    route = "partitioned" if over else "fused"
    for x, y in ((a, b), (b, a)):
        check_pair(engines, on, x, y, _oracle(x, y), (route, route), ("search", "search"),
                   ks_of=lambda n: sets[n])
