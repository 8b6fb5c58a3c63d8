"""A CPU model of launch_join2's choice of kernels (csrc/join.hip), and the inputs of
tests/test_gpu_join_variants.py (helper module: no tests).

dg_join2 runs one of 16 join2_stream_kernel<FAST, KEYED, CHG, LATE> instantiations -- the
fused launch (LATE: splits searched in the kernel, up to FUSE_IT tiles per workgroup) or the
partitioned one behind join2_partition_kernel -- or the two-pass pair join2_slot_kernel +
join2_compact_kernel; the fused kernel also picks one of two merge bodies from its VVs' node
ids.  From outside the library only the joined rows show, so WHICH of them a call runs is
decided here, by a restatement of the host's decisions.  tests/test_join_routes.py pins the
constants below to csrc/dg_launch.h and the units of the join and the model's answer for every
(engine, shape) pair of the GPU file, whose tests assert through route() that each call
lands where it is meant to.

Modelled: an engine with DG_JOIN_WORKERS = workers > 0, where nothing depends on the
device, and the default engine (workers = 0) under the stated assumption that the resident
grid holds at least ntiles + 1 workgroups (DEFAULT_MAX_TILES bounds the shapes the model
answers for)."""
import functools

import numpy as np

from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.interning import splitmix64_np
from oracle import ref as R

VV, DOTS = W.VV, W.DOTS
TOP = (1 << 64) - 1

# ---------------------------------------------------------------- the constants (one table)
# csrc/dg_launch.h: DG_JOIN_BLOCK, DG_JOIN_ITEMS, JOIN_TILE = block * items - JOIN_TILE_LESS;
# csrc/dg_jtile.h: FUSE_IT, VT, KS, CQ = ceil(CQ_SPAN / block); csrc/api_join.hip: splice_wanted's
# factor.  (test_join_routes.py::test_constants_match_the_sources)
CONST = {"DG_JOIN_BLOCK": 512, "DG_JOIN_ITEMS": 2, "JOIN_TILE_LESS": 8, "FUSE_IT": 4, "VT": 64,
         "KS": 64, "CQ_SPAN": 1024, "SPLICE_FACTOR": 8}
JOIN_BLOCK, JOIN_ITEMS = CONST["DG_JOIN_BLOCK"], CONST["DG_JOIN_ITEMS"]
JOIN_TILE = JOIN_BLOCK * JOIN_ITEMS - CONST["JOIN_TILE_LESS"]
FUSE_IT, VT, KS = CONST["FUSE_IT"], CONST["VT"], CONST["KS"]
CQ = (CONST["CQ_SPAN"] + JOIN_BLOCK - 1) // JOIN_BLOCK
# the default engine sizes its grid from the occupancy query; the model assumes that at
# least this many join workgroups (and the context union's) are resident at once (an
# MI355X has 256 compute units, each of which holds at least one)
DEFAULT_MAX_TILES = 64

# The engines of the GPU file: environment at dg_engine_create, and the route a call of 21
# tiles is meant to take there, (dg_join2, dg_join2_changes).
ENGINES = {
    "default": ({}, ("fused", "fused")),
    "fused4": ({"DG_JOIN_WORKERS": "6"}, ("fused", "fused")),
    "part2": ({"DG_JOIN_WORKERS": "2"}, ("partitioned", "partitioned")),
    "part1": ({"DG_JOIN_WORKERS": "1"}, ("partitioned", "partitioned")),
    "twopass": ({"DG_JOIN_MODE": "2"}, ("two_pass", "fused")),
}


def engine_params(name):
    """(workers, two_pass) of a named engine, as dg_engine_create reads its environment."""
    env = ENGINES[name][0]
    return int(env.get("DG_JOIN_WORKERS", 0)), env.get("DG_JOIN_MODE", "")[:1] == "2"


def _ceil_div(a, b):
    return (a + b - 1) // b


def join2_tiles(na, nb):
    return _ceil_div(na + nb, JOIN_TILE)


def balance_tiles(total, ntiles, G):
    """balance_tiles: (jt, ntiles) re-cut so that every stripe of G tiles is full."""
    if G == 0 or ntiles <= G:
        return JOIN_TILE, ntiles
    k = _ceil_div(ntiles, G)
    jt = min((_ceil_div(total, k * G) + 1) & ~1, JOIN_TILE)
    return jt, _ceil_div(total, jt)


def route(na, nb, workers=0, two_pass=False, chg=False, keyed=False, kind_a=VV, kind_b=VV,
          vv_a=(), vv_b=()):
    """What launch_join2 launches for a join of na + nb rows.

    workers, two_pass: the engine's DG_JOIN_WORKERS (0: unset) and DG_JOIN_MODE=2; chg:
    dg_join2_changes (single pass whatever the mode); keyed: a key list; kind_a / kind_b and
    vv_a / vv_b: the contexts' kinds and, for a version vector, its node ids.

    Returns a dict:
      route    "fused" | "partitioned" | "two_pass" ("empty": no rows, only the context union)
      G        tile workgroups (two_pass: one per tile)
      jt       merged positions per tile after balance_tiles (JOIN_TILE when chg)
      ntiles   tiles
      stripes  iterations of a workgroup, ceil(ntiles / G)
      last     tiles of the last stripe (< G: workgroups past it leave the loop a tile early,
               and the fused split search meets its `tk >= ntiles` break)
      fast     both contexts are version vectors (the LDS tables)
      merge    "nofb" (the fused kernel's body without the coverage search: fast and no VV
               node id >= VT), "search" (any other fast case), "dots" (not fast)
      kernel   (FAST, KEYED, CHG, LATE) of the stream kernel, or ("slot", FAST, KEYED)"""
    total = na + nb
    ntiles, jt = join2_tiles(na, nb), JOIN_TILE
    fast = kind_a == VV and kind_b == VV
    if ntiles == 0:
        return dict(route="empty", G=0, jt=jt, ntiles=0, stripes=0, last=0, fast=fast, merge=None,
                    kernel=None)
    far = any(int(n) >= VT for n in vv_a) or any(int(n) >= VT for n in vv_b)
    if two_pass and not chg:
        return dict(route="two_pass", G=ntiles, jt=jt, ntiles=ntiles, stripes=1, last=ntiles, fast=fast,
                    merge="search" if fast else "dots", kernel=("slot", fast, keyed))
    if workers > 0:
        g = min(ntiles, workers, CQ * JOIN_BLOCK)
    else:
        assert ntiles <= DEFAULT_MAX_TILES, "the default engine is modelled for small joins only"
        g = ntiles
    # (workers > 0: gr = g + 1, so the fused grid gt = min(ntiles, gr - 1, CQ * JB) = g)
    fused = ntiles <= FUSE_IT * g
    if fused and not chg:
        jt, ntiles = balance_tiles(total, ntiles, g)
    stripes = _ceil_div(ntiles, g)
    merge = "dots" if not fast else "nofb" if fused and not far else "search"
    return dict(route="fused" if fused else "partitioned", G=g, jt=jt, ntiles=ntiles, stripes=stripes,
                last=ntiles - (stripes - 1) * g, fast=fast, merge=merge,
                kernel=(fast, keyed, chg, fused))


def splice_wanted(na, nb, n_keys):
    """api_join.hip's splice_wanted for aligned stores: the keyed join goes to the splice,
    not to the join kernels."""
    return n_keys > 0 and (n_keys + nb) * CONST["SPLICE_FACTOR"] <= na


def key_slices(ka, kb, keys, jt):
    """The keyset slice lengths km of every tile (key_split / kslice of the stream kernel):
    ksplit[q] = the first keyset index >= the key at merged position q * jt.  A tile with
    km <= KS stages its slice in LDS, a longer one searches the keyset in global memory."""
    merged = np.sort(np.concatenate([ka, kb]))
    keys = np.asarray(keys, np.uint64)
    total = len(merged)
    nt = _ceil_div(total, jt)
    d = np.minimum(np.arange(nt + 1, dtype=np.int64) * jt, total)
    ks = np.where(d < total, np.searchsorted(keys, merged[np.minimum(d, total - 1)]), len(keys))
    return np.minimum(ks[1:] + 1, len(keys)) - ks[:-1]


def route_of(engine, x, y, chg=False, keys=None):
    """route() of a call join(x, y, keys) on a named engine."""
    workers, two_pass = engine_params(engine)
    vv = [tuple(r["ctx"][1].tolist()) if r["ctx"][0] == VV else () for r in (x, y)]
    return route(len(x["rows"][0]), len(y["rows"][0]), workers=workers, two_pass=two_pass, chg=chg,
                 keyed=keys is not None, kind_a=x["ctx"][0], kind_b=y["ctx"][0], vv_a=vv[0], vv_b=vv[1])


# ---------------------------------------------------------------- inputs
# Node ids: the base pairs draw nodes 0..5; a monotone table relabels them (rows and
# contexts), so every store and context stays sorted and unique.
NEAR = np.arange(6, dtype=np.uint32)
FAR = np.array([0, 63, 64, 65, 1000, 2 ** 32 - 1], np.uint32)
# hand-made rows (below): a node under VT and one over it that no context names
LOW_ABSENT, FAR_ABSENT = 40, 70

BASES = {"vv_sparse": dict(dense_ctx=False, ctx_kind=VV), "vv_dense": dict(dense_ctx=True, ctx_kind=VV),
         "dots": dict(dense_ctx=False, ctx_kind=DOTS)}

# layout -> (base pair, node table, which sides' VVs lose their entries of node id >= VT,
#            which sides' dot sets become version vectors)
LAYOUTS = {
    "near":           ("vv_sparse", NEAR, "", ""),
    "far_both":       ("vv_sparse", FAR, "", ""),
    "far_rows_only":  ("vv_sparse", FAR, "ab", ""),
    "far_a_only":     ("vv_sparse", FAR, "b", ""),
    "far_b_only":     ("vv_sparse", FAR, "a", ""),
    "dense_near":     ("vv_dense", NEAR, "", ""),
    "dense_far_both": ("vv_dense", FAR, "", ""),
    "dots_dots":      ("dots", FAR, "", ""),
    "vv_dots":        ("dots", FAR, "", "a"),
    "dots_vv":        ("dots", FAR, "", "b"),
}
VV_LAYOUTS = [n for n, v in LAYOUTS.items() if v[0] != "dots"]
FAR_LAYOUTS = [n for n in VV_LAYOUTS if LAYOUTS[n][1] is FAR]
# the merge body on (a fused engine, any other engine)
MERGE = {n: ("dots", "dots") if v[0] == "dots" else
         ("nofb" if v[1] is NEAR or v[2] == "ab" else "search", "search") for n, v in LAYOUTS.items()}


@functools.lru_cache(maxsize=None)
def base_pair(base, n_keys=6000, seed=1):
    return W.random_pair(np.random.default_rng(seed), n_keys, n_nodes=6, ts_range=4, **BASES[base])


def _relabel(rep, table, drop_far, to_vv):
    rows = rep["rows"]
    kind, node, cnt = rep["ctx"]
    if to_vv:  # half of the side's own dots per node: covers some of both stores, not all
        top = {}
        for n, c in zip(rows[3].tolist(), rows[4].tolist()):
            top[n] = max(top.get(n, 0), c)
        kind, node, cnt = W.vv({n: c // 2 for n, c in top.items()})
    node = table[node]
    if drop_far:
        assert kind == VV
        m = node < VT
        node, cnt = node[m], cnt[m]
    return {"rows": rows[:3] + (table[rows[3]],) + rows[4:],
            "ctx": (kind, np.ascontiguousarray(node, np.uint32), np.ascontiguousarray(cnt, np.uint64))}


def _merge_rows(rows, extra):
    cols = W.sort_rows(*(np.concatenate([x, np.asarray(y, x.dtype)]) for x, y in zip(rows, extra)))
    same = np.ones(len(cols[0]) - 1, bool)
    for c in cols:
        same &= c[1:] == c[:-1]
    assert not same.any()
    return cols


def extra_keys(side, kind):
    """The 8 keys of one kind of hand-made row (side 0 / 1 / 2: a only, b only, both)."""
    return splitmix64_np(np.uint64(1 << 50) + np.arange(8, dtype=np.uint64) + np.uint64(64 * side + 8 * kind))


EXTRA_KINDS = [(LOW_ABSENT, 0), (FAR_ABSENT, 0), (LOW_ABSENT, 1), (FAR_ABSENT, 1), (1000, 0)]


def _extras(side):
    """Hand-made rows on 8 new keys per kind: dot counter 0 on a node below VT that no
    context names, on one of VT or more, counter 1 on the same two nodes, and counter 0 on
    node 1000 (in the far VVs).  Map.get(vv, n, 0) >= 0: a version vector covers every
    counter-0 dot, named node or not (the oracle's ctx_member agrees); a dot set covers none
    of these.  Side 2's rows are in both stores and stay whatever covers them."""
    key, node, cnt = [], [], []
    for kind, (nd, c) in enumerate(EXTRA_KINDS):
        ks = extra_keys(side, kind)
        key.append(ks)
        node.append(np.full(len(ks), nd, np.uint32))
        cnt.append(np.full(len(ks), c, np.uint64))
    key, node, cnt = np.concatenate(key), np.concatenate(node), np.concatenate(cnt)
    n = len(key)
    return (key, np.full(n, (1 << 62) + 9, np.uint64), np.arange(n, dtype=np.int64) % 3 - 1, node, cnt)


@functools.lru_cache(maxsize=None)
def layout(name):
    """The pair (a, b) of a layout: the base pair relabelled, plus the hand-made rows."""
    base, table, drop, to_vv = LAYOUTS[name]
    out = []
    for side, rep in zip("ab", base_pair(base)):
        r = _relabel(rep, table, side in drop, side in to_vv)
        rows = _merge_rows(_merge_rows(r["rows"], _extras("ab".index(side))), _extras(2))
        out.append({"rows": rows, "ctx": r["ctx"]})
    return tuple(out)


def union_keys(a, b):
    return np.unique(np.concatenate([a["rows"][0], b["rows"][0], np.zeros(0, np.uint64)]))


def keysets(a, b):
    """half: every second key of the union (more than KS keys per tile: the keyset is
    searched in global memory); sparse: every 40th key plus absent keys, 0 and 2^64 - 1
    among them (a few per tile: the LDS slice)."""
    keys = union_keys(a, b)
    rng = np.random.default_rng(len(keys))
    near = keys[rng.integers(0, len(keys), 40)]
    near = near[near != np.uint64(TOP)] + np.uint64(1)
    cand = np.concatenate([near, rng.integers(0, 1 << 64, 40, dtype=np.uint64), np.array([0, TOP], np.uint64)])
    return {"half": keys[::2], "sparse": np.union1d(keys[5::40], np.setdiff1d(cand, keys))}


KEYSETS = (None, "half", "sparse")


def keyset(a, b, ks_name):
    return None if ks_name is None else keysets(a, b)[ks_name]


@functools.lru_cache(maxsize=None)
def expected(name, order, ks_name):
    """The oracle's (rows, context, changed keys) of a layout's call, computed once."""
    a, b = layout(name)
    x, y = (a, b) if order == "ab" else (b, a)
    ks = keyset(a, b, ks_name)
    rows, ctx = R.join2(x["rows"], x["ctx"], y["rows"], y["ctx"], keys=ks)
    return rows, ctx, R.changed_keys(x["rows"], rows, ks)


def _distinct_far(x, y):
    """Distinct rows of node id >= VT in the two stores together."""
    cols = W.sort_rows(*(np.concatenate([p, q]) for p, q in zip(x, y)))
    same = np.ones(len(cols[0]) - 1, bool)
    for c in cols:
        same &= c[1:] == c[:-1]
    return int((cols[3] >= VT).sum() - (cols[3][1:][same] >= VT).sum())


@functools.lru_cache(maxsize=None)
def input_conditions(name):
    """The conditions the GPU tests rely on, checked on the oracle's results: every call
    keeps and drops rows; in the far layouts rows of node id >= VT are kept and dropped;
    counter-0 rows on a far node are dropped on VV layouts (and some of their keys lie
    inside and some outside the every-second-key keyset); keyed calls have changed keys
    inside the keyset and differences outside it.  Returns the figures:
    (order, keyset) -> (rows of x, rows of y, rows out, changed keys), and
    (order, "far") -> (distinct rows in of node id >= VT, such rows out)."""
    a, b = layout(name)
    out = {}
    for order in ("ab", "ba"):
        x, y = (a, b) if order == "ab" else (b, a)
        nx, ny = len(x["rows"][0]), len(y["rows"][0])
        for ks_name in KEYSETS:
            rows, _, changed = expected(name, order, ks_name)
            ks = keyset(a, b, ks_name)
            assert 0 < len(rows[0]) < nx + ny, (name, order, ks_name)
            if ks is not None:
                assert not splice_wanted(nx, ny, len(ks)), (name, order, ks_name)
                full = R.changed_keys(x["rows"], rows, None)
                assert len(changed) > 0 and len(full) > len(changed), (name, order, ks_name)
            out[(order, ks_name)] = (nx, ny, len(rows[0]), len(changed))
        rows = expected(name, order, None)[0]
        if name in FAR_LAYOUTS:
            far_in = _distinct_far(x["rows"], y["rows"])
            far_out = int((rows[3] >= VT).sum())
            assert 0 < far_out < far_in, (name, order, far_out, far_in)
            out[(order, "far")] = (far_in, far_out)
        if name in VV_LAYOUTS:
            # the x-only counter-0 rows on FAR_ABSENT are dropped, the counter-1 ones kept
            side = 0 if order == "ab" else 1
            zero, one = extra_keys(side, 1), extra_keys(side, 3)
            assert not np.isin(zero, rows[0]).any() and np.isin(one, rows[0]).all()
            assert np.isin(extra_keys(2, 1), rows[0]).all()  # in both stores: kept
            # (keyed with every second key: some of them joined, some carried)
            assert 0 < int(np.isin(zero, keysets(a, b)["half"]).sum()) < len(zero)
    return out


# ---------------------------------------------------------------- edges
def _cut(rep, n):
    return {"rows": tuple(np.ascontiguousarray(c[:n]) for c in rep["rows"]), "ctx": rep["ctx"]}


@functools.lru_cache(maxsize=None)
def edges():
    """Far VVs throughout: a empty, b empty, both empty (the context union alone), one row
    each."""
    a, b = layout("far_both")
    return {"a_empty": (_cut(a, 0), b), "b_empty": (a, _cut(b, 0)), "both_empty": (_cut(a, 0), _cut(b, 0)),
            "one_row_each": (_cut(a, 1), _cut(b, 1))}


BOUNDARY_ENGINES = ("fused4", "part2")


@functools.lru_cache(maxsize=None)
def boundary(engine, over):
    """A pair of exactly FUSE_IT * G tiles (over = 0: the largest fused launch, every tile
    full) or one row more (over = 1: the partitioned launch, its last tile one row), for an
    engine of G workers: prefixes of a far_both-relabelled pair."""
    G = engine_params(engine)[0]
    total = FUSE_IT * G * JOIN_TILE + over
    a, b = (_relabel(r, FAR, False, False) for r in base_pair("vv_sparse", 7400, 2))
    na_all, nb_all = len(a["rows"][0]), len(b["rows"][0])
    assert na_all + nb_all >= total
    na = total * na_all // (na_all + nb_all)
    return _cut(a, na), _cut(b, total - na)


def shapes():
    """Every (label, a, b) the GPU file joins (each also in the other order)."""
    out = [(name,) + layout(name) for name in LAYOUTS]
    out += [(name,) + pair for name, pair in edges().items()]
    out += [("boundary_%s_%d" % (e, o),) + boundary(e, o) for e in BOUNDARY_ENGINES for o in (0, 1)]
    return out
