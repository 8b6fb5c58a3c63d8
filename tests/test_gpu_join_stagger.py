"""The stream join's prefix wait (csrc/join_stream.hip, dg_jstripe.h): a workgroup waits for
the counts of the tiles [t - G, t) before it writes tile t -- the positions below its own in
t's stripe and the rest of the stripe before -- and no longer for the whole stripe.

Pairs of about 40, 37 and 21 tiles on engines of DG_JOIN_WORKERS = 1, 2, 3, 6 and 7: odd and
even grids, halves of unequal size, 6 to 40 stripes on the partitioned kernel, three and four
fused iterations on 7 and 6 workgroups, a last stripe that holds tiles of the lower half
only.  Each with DG_JOIN_STAGGER (a delay of the upper half of every stripe before its first
tile) at 0, unset and several iterations long: behind a delayed upper half the lower half
meets the wait for the older counts.  Version-vector, dot-set and mixed contexts, a keyed
join, change events, an empty side.  Every result is bit-exact against the same call on a
DG_JOIN_MODE=2 engine and against the C oracle; tests/join_routes.py says where each call
goes.  One join on DG_JOIN_WORKERS=1024, a grid that cannot be resident, must equal the
co-resident one through the abort and re-run."""
import functools
import os

import numpy as np
import pytest

import join_routes as J
from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.store import Engine
from oracle import ref as R
from test_gpu_join_variants import check_call
from test_gpu_parity import up

pytestmark = pytest.mark.gpu

WORKERS = (1, 2, 3, 6, 7)
STAGGERS = {"none": "0", "default": None, "long": "120"}  # long: ~30 us, several iterations


def _engine(env):
    os.environ.update(env)
    try:
        return Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(workers, stagger):
        key = (workers, stagger)
        if key not in made:
            env = {"DG_JOIN_WORKERS": str(workers)} if workers else {"DG_JOIN_MODE": "2"}
            if STAGGERS.get(stagger) is not None:
                env["DG_JOIN_STAGGER"] = STAGGERS[stagger]
            made[key] = _engine(env)
        return made[key]

    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def big(base):
    """A pair of about 20,000 rows a side (40 tiles): `vv`, `dots`, or `mixed` (a's dot set
    replaced by a version vector of half its dots)."""
    a, b = J.base_pair({"vv": "vv_sparse", "dots": "dots", "mixed": "dots"}[base], 12000, 3)
    if base == "mixed":
        a = J._relabel(a, J.NEAR, False, True)
    return a, b


@functools.lru_cache(maxsize=None)
def cut37():
    """The version-vector pair cut to 37 tiles: 37 mod G <= ceil(G / 2) for every G of
    WORKERS, so the last stripe holds tiles of the lower half only."""
    a, b = big("vv")
    na_all, nb_all = len(a["rows"][0]), len(b["rows"][0])
    total = 36 * J.JOIN_TILE + 500
    assert na_all + nb_all >= total
    na = total * na_all // (na_all + nb_all)
    return J._cut(a, na), J._cut(b, total - na)


def pairs():
    a, b = big("vv")
    return {"vv": big("vv"), "dots": big("dots"), "mixed": big("mixed"), "cut37": cut37(),
            "fused21": J.layout("near"), "a_empty": (J._cut(a, 0), b), "b_empty": (a, J._cut(b, 0))}


@functools.lru_cache(maxsize=None)
def case(name, keyed):
    """(x, y, keys, the oracle's rows / context / changed keys), computed once."""
    x, y = pairs()[name]
    ks = J.union_keys(x, y)[::2] if keyed else None
    rows, ctx = R.join2(x["rows"], x["ctx"], y["rows"], y["ctx"], keys=ks)
    return x, y, ks, (rows, ctx, R.changed_keys(x["rows"], rows, ks))


# (pair, keyed, change events)
CALLS = [("vv", False, False), ("dots", False, False), ("mixed", False, False), ("vv", True, False),
         ("vv", False, True), ("vv", True, True), ("cut37", False, False), ("cut37", False, True),
         ("fused21", False, False), ("fused21", False, True), ("a_empty", False, False),
         ("b_empty", False, True)]


def _route(x, y, workers, chg, keyed):
    vv = [tuple(r["ctx"][1].tolist()) if r["ctx"][0] == J.VV else () for r in (x, y)]
    return J.route(len(x["rows"][0]), len(y["rows"][0]), workers=workers, chg=chg, keyed=keyed,
                   kind_a=x["ctx"][0], kind_b=y["ctx"][0], vv_a=vv[0], vv_b=vv[1])


def test_shapes():
    """The shapes are what the docstring says (the model's answer, no GPU call)."""
    for w in WORKERS:
        ge = (w + 1) // 2
        for name, n in (("vv", 40), ("dots", 40), ("mixed", 40)):
            x, y = pairs()[name]
            r = _route(x, y, w, False, False)
            assert r["route"] == "partitioned" and abs(r["ntiles"] - n) <= 3, (w, name, r)
            assert r["stripes"] >= 6
        x, y = pairs()["cut37"]
        for chg in (False, True):
            r = _route(x, y, w, chg, False)
            assert r["route"] == "partitioned" and r["ntiles"] == 37 and 0 < r["last"] <= ge, (w, r)
        x, y = pairs()["fused21"]
        r = _route(x, y, w, False, False)
        assert r["route"] == ("fused" if w >= 6 else "partitioned"), (w, r)
        if w >= 6:
            assert r["stripes"] == (4 if w == 6 else 3) and r["merge"] == "nofb", (w, r)
            assert _route(x, y, w, True, False)["route"] == "fused"


@pytest.mark.parametrize("stagger", list(STAGGERS))
@pytest.mark.parametrize("workers", WORKERS)
def test_prefix_wait(engines, workers, stagger):
    eng, two = engines(workers, stagger), engines(0, None)
    for name, keyed, chg in CALLS:
        x, y, ks, want = case(name, keyed)
        r = _route(x, y, workers, chg, keyed)
        assert r["route"] in ("fused", "partitioned") and r["G"] == min(workers, r["ntiles"]), (name, r)
        dev = up(x) + up(y)
        what = (workers, stagger, name, "keyed" if keyed else "all", "changes" if chg else "join2", r["route"])
        check_call(eng, dev, ks, chg, want, what)
        check_call(two, dev, ks, chg, want, what + ("two-pass engine",))


@pytest.mark.parametrize("stagger", ["default", "long"])
def test_overscheduled_grid(stagger, monkeypatch):
    """DG_JOIN_WORKERS=1024 on about 1,250 tiles: half the grid cannot start, the resident
    half gives up its waits by stripe position and the join re-runs; rows and context equal
    the co-resident grid's."""
    from delta_crdt_ex_amd.store import Context, Store
    dev = "cuda:0"
    a, b = W.config5(n_keys=700_000, n_nodes=64, seed=77)
    sa, sb = Store.from_numpy(*a["rows"], device=dev), Store.from_numpy(*b["rows"], device=dev)
    ca, cb = Context.from_numpy(*a["ctx"], dev), Context.from_numpy(*b["ctx"], dev)
    assert J.join2_tiles(sa.n, sb.n) > 1024
    ref = Engine(0)
    want_out, want_ctx = ref.join2(sa, ca, sb, cb)
    want = tuple(c.copy() for c in want_out.to_numpy()) + tuple(c.copy() for c in want_ctx.to_numpy())
    ref.close()
    monkeypatch.setenv("DG_JOIN_WORKERS", "1024")
    if STAGGERS[stagger] is not None:
        monkeypatch.setenv("DG_JOIN_STAGGER", STAGGERS[stagger])
    eng = Engine(0)
    out, octx = eng.join2(sa, ca, sb, cb)
    for g, w in zip(tuple(out.to_numpy()) + tuple(octx.to_numpy()), want):
        assert np.array_equal(g, w)
    eng.close()
