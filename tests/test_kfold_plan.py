"""The CPU model of the one-pass fold's bucket plan (tests/kfold_plan.py): pinned to the
constants of csrc/dg_launch.h, self-consistent, and -- for every input that
tests/test_gpu_kfold_seams.py runs -- the REACH assertion: the model sends that input down
the path the GPU test is for (first attempt, the retry, refusal; which overflow site; a
thread's second staged item; one sub-bucket; the probe wrap).  From outside the library only
accept or refuse shows, so these assertions are what ties a GPU case to a code path.  Also
the generators' outputs as stores, and the C oracle's fold against the term oracle on the
small ones, so the reference the GPU is held to is itself checked on these shapes."""
import hashlib
import os
import re

import numpy as np
import pytest

import kfold_plan as P
from kfold_cases import DOTS, random_fold
from oracle import awlww_term as T
from oracle import ref as R
from test_c_oracle import ctx_equal, rows_equal, soa_to_term, term_to_soa_raw

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "delta_crdt_ex_amd", "csrc")


# ---------------------------------------------------------------- the model is the header's

def test_constants_match_the_header():
    """kfold_plan.CONST restates csrc/dg_launch.h (and kfold.hip's NSUB, CU, CUL): if a
    capacity, a mean or a limit moves there, the model is wrong until it follows."""
    h = open(os.path.join(CSRC, "dg_launch.h")).read()
    k = open(os.path.join(CSRC, "kfold.hip")).read()
    got = {}
    for name in ("DG_KFOLD_SCALE", "DG_KFOLD_BLOCK"):
        got[name] = int(re.search(r"#define\s+%s\s+(\d+)" % name, h).group(1))
    for name in ("KFOLD_CAP_S", "KFOLD_CAP_D", "KFOLD_CAP_M", "KFOLD_MEAN_S", "KFOLD_MEAN_D",
                 "KFOLD_MEAN_M", "KFOLD_MEAN_U"):
        got[name] = int(re.search(r"\b%s\s*=\s*(\d+)\s*>>\s*DG_KFOLD_SCALE\b" % name, h).group(1))
    for name in ("KFOLD_MAX_K", "KNT"):
        got[name] = int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, h).group(1))
    m = re.search(r"KF_CNT_LIMIT\s*=\s*\(1ull\s*<<\s*(\d+)\)\s*-\s*1\s*;", h)
    got["KF_CNT_LIMIT"] = (1 << int(m.group(1))) - 1
    got["DG_KFOLD_NSUB"] = int(re.search(r"#define\s+DG_KFOLD_NSUB\s+(\d+)", k).group(1))
    assert got == P.CONST, "csrc/dg_launch.h moved: tests/kfold_plan.py's model must follow it"
    assert re.search(r"KFOLD_BLOCK\s*=\s*DG_KFOLD_BLOCK\s*;", h)
    assert re.search(r"constexpr\s+int\s+CU\s*=\s*CD\s*\+\s*CM\s*;", k)
    assert re.search(r"constexpr\s+int\s+CUL\s*=\s*CD\s*\+\s*2\s*\*\s*CM\s*;", k)
    # the two overflow predicates and the retry factor, as the model restates them
    assert "nS > (u32)CS || nD > (u32)CD || nU > (u32)CUL || nU - nD > (u32)(CUL - CD)" in k
    assert "nD + n_keep > (u32)CU" in k
    assert "T0 << (3 * attempt)" in open(os.path.join(CSRC, "api_fold.hip")).read()
    assert (P.CS, P.CD, P.CU, P.CUL, P.KB) == (1024, 512, 1024, 1536, 1024)


def _checksum(st, ds):
    h = hashlib.sha256()
    for c in st["rows"] + tuple(st["ctx"][1:]):
        h.update(np.ascontiguousarray(c).tobytes())
    h.update(bytes([st["ctx"][0]]))
    for d in ds:
        for c in d["rows"] + tuple(d["ctx"][1:]):
            h.update(np.ascontiguousarray(c).tobytes())
        h.update(bytes([d["ctx"][0]]))
        h.update(b"full" if d["keys"] is None else d["keys"].tobytes())
    return h.hexdigest()[:16]


# recorded on the commit before random_fold gained keys=
SEEDS = [
    (dict(seed=0, n_keys=3000, k=1), "49ceb23463c7ca15"),
    (dict(seed=4, n_keys=3000, k=64), "f936aaef87a29a65"),
    (dict(seed=10, n_keys=400, k=24, rows_per_key=8, p_keys=0.4, p_take=0.8, p_outside=0.05),
     "58f8faa54a50d536"),
    (dict(seed=20, n_keys=2000, k=12, p_full=0.3), "60d2686a5dcbb1b7"),
    (dict(seed=31, n_keys=3000, k=6, hashed=False), "21d3e7d084449451"),
    (dict(seed=32, n_keys=800, k=5, dots_ctx=True), "d2ce2efe0eded005"),
    (dict(seed=50, n_keys=2000, k=12, delta_dots=True), "03c90a331453bccd"),
    (dict(seed=22, n_keys=2000, k=8, n_nodes=40, node_base=1000, ctx_node_max=1024), "6089fe56db4c9fcd"),
]


@pytest.mark.parametrize("kw,want", SEEDS, ids=[str(i) for i in range(len(SEEDS))])
def test_random_fold_seeds_unchanged(kw, want):
    """The keys= argument changed no draw: every existing seed gives the arrays it gave."""
    assert _checksum(*random_fold(**kw)) == want


def test_random_fold_keys_argument():
    """keys= replaces the key ids and nothing else (the rows re-sort by the new keys)."""
    st, ds = random_fold(5, n_keys=300, k=3)
    ids = np.arange(1, 301, dtype=np.uint64)
    st2, ds2 = random_fold(5, keys=P.splitmix64_np(ids), k=3)
    assert _checksum(st, ds) == _checksum(st2, ds2)
    st3, ds3 = random_fold(5, keys=ids * np.uint64(7), k=3)
    st4, ds4 = random_fold(5, n_keys=300, k=3, hashed=False)
    assert np.array_equal(st3["rows"][0], st4["rows"][0] * np.uint64(7))
    assert all(np.array_equal(a, b) for a, b in zip(st3["rows"][1:], st4["rows"][1:]))
    assert all(np.array_equal(a["keys"], b["keys"] * np.uint64(7)) for a, b in zip(ds3, ds4))


# ---------------------------------------------------------------- the model itself

def test_mulhi_is_exact():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.integers(0, 1 << 64, 500, dtype=np.uint64),
                        np.array([0, 1, P.TOP - 1, P.TOP, 1 << 32, (1 << 32) - 1], np.uint64)])
    for b in (1, 2, 9, 88, 1024, 88 * 1024, (1 << 31) - 1, ((1 << 31) - 1) * 1024, P.TOP):
        assert P.mulhi(a, b).tolist() == [(int(x) * b) >> 64 for x in a]


@pytest.mark.parametrize("T", [1, 2, 9, 72, 1000])
def test_plan_is_self_consistent(T):
    st, ds = P.ends()
    p = P.plan(st, ds, T)
    assert len(p) == T
    assert sum(b["nS"] for b in p) == len(st["rows"][0])
    assert sum(b["nD"] for b in p) == sum(len(d["rows"][0]) for d in ds)
    assert sum(b["nM"] for b in p) == sum(len(d["keys"]) for d in ds)
    assert sum(b["n_keep"] for b in p) == sum(int((~np.isin(d["keys"], d["rows"][0])).sum()) for d in ds)
    assert all(b["n_keep"] <= b["nM"] and b["max_sub"] <= b["nD"] + b["n_keep"] and
               b["max_sub_s"] <= b["nS"] for b in p)
    assert P.bucket_of(np.array([0, P.TOP], np.uint64), T).tolist() == [0, T - 1]
    b, s = P.sub_of(np.array([0, P.TOP], np.uint64), T)
    assert (b.tolist(), s.tolist()) == ([0, T - 1], [0, P.NSUB - 1])
    # every key of bucket t lies in [ceil(t 2^64 / T), ceil((t + 1) 2^64 / T))
    keys = st["rows"][0]
    for key, t in zip(keys[::97].tolist(), P.bucket_of(keys[::97], T).tolist()):
        assert -((-t << 64) // T) <= key < -((-(t + 1) << 64) // T)


def test_t0_terms():
    """Every term of kfold_pass's formula decides alone; full deltas count no keys."""
    def fold(n_s, rows, keys):
        z = np.zeros
        return ({"rows": (z(n_s, np.uint64),) * 5, "ctx": (0, z(0), z(0))},
                [{"rows": (z(rows, np.uint64),) * 5, "ctx": None, "keys": None if keys is None else z(keys)}])
    assert P.t0(*fold(0, 0, 0)) == 1
    assert P.t0(*fold(800, 400, 800)) == 1
    assert P.t0(*fold(801, 0, 0)) == 2
    assert P.t0(*fold(0, 401, 0)) == 2
    assert P.t0(*fold(0, 0, 801)) == 2
    assert P.t0(*fold(0, 400, 801)) == 2
    assert P.t0(*fold(0, 401, 800)) == 2
    assert P.t0(*fold(0, 400, None)) == 1


# ---------------------------------------------------------------- reach: the existing suite

@pytest.mark.parametrize("seed,k", [(0, 1), (1, 3), (2, 8), (3, 17), (4, 64)])
def test_onepass_random_is_first_attempt(seed, k):
    assert P.verdict(*random_fold(seed, n_keys=3000, k=k)) == "first"


def test_crowded_keys_reach_the_retry():
    """What test_gpu_kfold.py::test_onepass_crowded_keys really does: all three seeds overflow
    on delta rows (nD > 512 and nothing else) in some buckets at T0 and fit at 8 T0."""
    seen = {}
    for seed in (10, 11, 12):
        st, ds = random_fold(seed, n_keys=400, k=24, rows_per_key=8, p_keys=0.4, p_take=0.8,
                             p_outside=0.05)
        tr = P.trace_pass(st, ds)
        assert tr["verdict"] == "retry" and not tr["attempts"][0]["second"]
        p = P.plan(st, ds, tr["T0"])
        assert {p[t]["why"] for t in tr["attempts"][0]["first"]} <= {"D", "DU"}
        seen[seed] = (tr["T0"], len(tr["attempts"][0]["first"]))
    assert seen == {10: (38, 7), 11: (37, 8), 12: (39, 6)}, seen


# ---------------------------------------------------------------- reach: at the capacities

@pytest.mark.parametrize("layout", ["one", "many"])
def test_at_capacity_reach(layout):
    """Bucket 0 exactly at every capacity, accepted at T0 = 2 with 512 second items."""
    st, ds = P.at_capacity(layout=layout)
    assert len(ds) == {"one": 1, "many": 64}[layout]
    n_s, rows, keys = len(st["rows"][0]), sum(len(d["rows"][0]) for d in ds), sum(len(d["keys"]) for d in ds)
    # T0 = 2 by all four terms
    assert [-(-n_s // 800), -(-rows // 400), -(-keys // 800), -(-(rows + keys) // 1200)] == [2, 2, 2, 2]
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] == 2 and tr["attempts"][0]["q2"] == [0]
    b0, b1 = P.plan(st, ds, 2)
    assert (b0["nS"], b0["nD"], b0["nM"], b0["n_keep"]) == (1024, 512, 1024, 512)
    assert b0["nD"] + b0["nM"] == P.CUL and b0["nD"] + b0["n_keep"] == P.CU
    assert b0["nD"] + b0["nM"] - P.KB == 512  # threads 0..511 stage a second item
    assert 90 <= b1["nS"] <= 120 and (b1["nD"], b1["nM"], b1["n_keep"]) == (8, 6, 3)
    if layout == "many":
        assert all(len(d["rows"][0]) in (8, 9) and len(d["keys"]) in (16, 17) for d in ds)
    # the state and the deltas share tuples, and the deltas bring tuples the state lacks
    distinct = len(P.merge_rows(st["rows"], *[d["rows"] for d in ds])[0])
    assert n_s + 100 < distinct < n_s + rows - 100


WANT_OVER = {"S": (1025, 512, 1024, 512), "D": (1024, 513, 1023, 511), "M": (1024, 511, 1025, 514),
             "keep": (1024, 512, 1024, 513)}


@pytest.mark.parametrize("layout", ["one", "many"])
@pytest.mark.parametrize("over", P.OVERS)
def test_over_capacity_reach(over, layout):
    """One element over in ONE dimension: exactly that term of the first overflow site fires
    (or, for "keep", no first-site term and the second site); packed below 2^60 both attempts
    overflow, spread over [0, 2^63) the retry fits."""
    for spread in (False, True):
        st, ds = P.at_capacity(over, spread, layout)
        tr = P.trace_pass(st, ds)
        assert tr["T0"] == 2 and tr["verdict"] == ("retry" if spread else "refuse")
        b0 = P.plan(st, ds, 2)[0]
        assert (b0["nS"], b0["nD"], b0["nM"], b0["n_keep"]) == WANT_OVER[over]
        assert b0["nD"] + b0["nM"] <= P.CUL
        a0, a1 = tr["attempts"]
        if over == "keep":
            assert not b0["first"] and b0["why"] == "" and b0["second"] and b0["q2"]
            assert (a0["first"], a0["second"]) == ([], [0])
            assert (a1["first"], a1["second"]) == ([], [] if spread else [0])
        else:
            assert b0["why"] == over and not b0["second"]
            assert (a0["first"], a0["second"]) == ([0], [])
            assert (a1["first"], a1["second"]) == ([] if spread else [0], [])
        assert a1["T"] == 16
        if not spread:  # bucket 0 of T = 16 holds what bucket 0 of T = 2 held
            b16 = P.plan(st, ds, 16)[0]
            assert (b16["nS"], b16["nD"], b16["nM"]) == (b0["nS"], b0["nD"], b0["nM"])


# ---------------------------------------------------------------- reach: rekeyed folds

@pytest.mark.parametrize("name", list(P.SKEW_CASES))
def test_rekeyed_reach(name):
    gen, seed, n_keys, k, kw, want = P.SKEW_CASES[name]
    st, ds = P.skew_case(name)
    assert n_keys <= 6000 and k <= 8
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == want and tr["host"] is None
    if want == "retry":
        a0, a1 = tr["attempts"]
        assert a0["first"] and not a0["second"] and not a1["first"] and not a1["second"]
    if want == "refuse":
        assert all(a["first"] for a in tr["attempts"])
    if kw.get("delta_dots"):
        assert all(d["ctx"][0] == DOTS for d in ds)
    if kw.get("p_full"):
        assert any(d["keys"] is None for d in ds) and any(d["keys"] is not None for d in ds)
    # the rekeying kept the fold: same shapes, same non-key columns
    st0, ds0 = random_fold(seed, n_keys=n_keys, k=k, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(st["rows"][1:], st0["rows"][1:]))
    assert [len(d["rows"][0]) for d in ds] == [len(d["rows"][0]) for d in ds0]


def test_dense_part_overflows_on_state_rows():
    """The dense sixteenth / eighth: one bucket over at T0, on STATE rows (a dimension no
    older input overflows on), none over at 8 T0."""
    seen = {}
    for name in ("dense_half_16th", "dense_third_8th"):
        st, ds = P.skew_case(name)
        tr = P.trace_pass(st, ds)
        p = P.plan(st, ds, tr["T0"])
        over = tr["attempts"][0]["first"]
        assert over == [0] and "S" in p[0]["why"]
        seen[name] = (tr["T0"], p[0]["nS"], max(b["nS"] for b in P.plan(st, ds, 8 * tr["T0"])))
    assert all(s > P.CS >= s8 for _, s, s8 in seen.values()), seen


def test_small_skewed_sets_sit_in_few_sub_buckets():
    """The small skewed folds fit their buckets whatever the keys: the skew is inside.
    dense_plus_max (keys 3 i): one sub-bucket holds all but the largest key's elements;
    two_clusters at T0 = 2: bucket 0's elements all in sub-bucket 0, bucket 1's in 1023."""
    st, ds = P.skew_case("dense_plus_max small")
    (b,) = P.plan(st, ds, 1)
    assert b["max_sub"] >= b["nD"] + b["n_keep"] - 8 and b["max_sub_s"] >= b["nS"] - 3
    st, ds = P.skew_case("two_clusters small")
    for b in P.plan(st, ds, 2):
        assert b["nS"] > 200 and b["max_sub"] == b["nD"] + b["n_keep"] and b["max_sub_s"] == b["nS"]
    assert set(P.sub_of(st["rows"][0], 2)[1].tolist()) == {0, P.NSUB - 1}


# ---------------------------------------------------------------- reach: inside a bucket

def test_one_sub_bucket_reach():
    st, ds = P.one_sub_bucket()
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] == 1
    (b,) = P.plan(st, ds, 1)
    assert b["max_sub"] == b["nD"] + b["n_keep"] > 400 and b["max_sub_s"] == b["nS"] > 400


def test_one_key_bucket_reach():
    st, ds = P.one_key_bucket()
    assert len(np.unique(np.concatenate([st["rows"][0]] + [d["rows"][0] for d in ds]))) == 1
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] == 2
    b0, b1 = P.plan(st, ds, 2)
    assert (b0["nS"], b0["nD"], b0["n_keep"]) == (P.CS, P.CD, 1) and b0["max_sub"] == P.CD + 1
    assert (b1["nS"], b1["nD"], b1["nM"]) == (0, 0, 0)
    full = [d["keys"] is None for d in ds]
    assert any(full) and not all(full) and len(ds[1]["keys"]) == 0 and len(ds[9]["rows"][0]) == 0
    # tuples shared between the state and the deltas, and between deltas
    allrows = P.merge_rows(st["rows"], *[d["rows"] for d in ds])
    assert len(allrows[0]) < P.CS + P.CD - 100


def test_ends_reach():
    st, ds = P.ends()
    assert P.ends_present(st, ds)
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] > 2
    assert P.bucket_of(P.END_KEYS, tr["T0"]).tolist() == [0, 0, tr["T0"] - 1, tr["T0"] - 1]


def test_all_runs_one_bucket_reach():
    st, ds = P.all_runs_one_bucket()
    assert len(ds) == P.MAX_K
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] == 1  # so all 128 runs meet in bucket 0
    for d in ds:
        assert len(d["rows"][0]) >= 1 and (~np.isin(d["keys"], d["rows"][0])).sum() >= 1
        assert (~np.isin(d["rows"][0], d["keys"])).sum() >= 1  # and a carried row
    # a key that delta 63 has rows of, another delta names and the state holds: bit 63 of R
    # and M set beside lower bits of K on a state candidate
    k63 = ds[63]["rows"][0]
    named = np.concatenate([d["keys"] for d in ds[:63]])
    assert np.any(np.isin(k63, named) & np.isin(k63, st["rows"][0]))
    assert np.any(~np.isin(ds[63]["keys"], k63))  # delta 63's kept entry: bit 63 of K


def test_gaps_reach():
    st, ds = P.gaps()
    tr = P.trace_pass(st, ds)
    assert tr["verdict"] == "first" and tr["T0"] == 8
    p = P.plan(st, ds, 8)
    assert [b["nS"] > 0 for b in p] == [t == 5 for t in range(8)]   # the state in one bucket
    assert [b["nD"] + b["nM"] > 0 for b in p] == [t != 5 for t in range(8)]
    for col in (ds[4]["rows"][0], ds[4]["keys"]):  # delta 4's runs: buckets 0 and 7 only
        assert set(P.bucket_of(col, 8).tolist()) == {0, 7}
    assert len(ds[5]["rows"][0]) == 0 and len(ds[5]["keys"]) == 0


def test_tiny_absent_keys_reach():
    st, ds = P.tiny_absent_keys()
    assert P.trace_pass(st, ds)["T0"] == 1 and P.verdict(st, ds) == "first"
    held = np.concatenate([st["rows"][0]] + [d["rows"][0] for d in ds])
    assert len(ds[0]["keys"]) == 40 and not np.isin(ds[0]["keys"], held).any()


# ---------------------------------------------------------------- reach: dot sets

@pytest.mark.parametrize("case", list(P.DOT_CASES))
def test_dot_edges_reach(case):
    st, ds, dots = P.dot_edges(case)
    assert all(d["ctx"][0] == DOTS for d in ds) and P.dset_size(ds) == 1024
    tr = P.trace_pass(st, ds)
    if P.DOT_CASES[case] == "refuse":
        assert tr["verdict"] == "refuse" and tr["host"] is not None
    else:
        assert tr["verdict"] == "first"
    # every extra dot is a state row on a key delta 1 names and has no row of
    d1 = ds[P.WRAP_DELTA]
    for node, cnt, in_ctx in dots:
        (i,) = np.flatnonzero((st["rows"][3] == node) & (st["rows"][4] == np.uint64(cnt)))
        key = st["rows"][0][i]
        assert key in d1["keys"] and key not in d1["rows"][0]
        assert in_ctx == bool(np.any((d1["ctx"][1] == node) & (d1["ctx"][2] == np.uint64(cnt))))
    want = {"counter 2^48-2": (7, (1 << 48) - 2), "counter 2^48-1": (7, (1 << 48) - 1),
            "node 1023": (1023, 9), "node 1024": (1024, 9)}.get(case)
    if want:
        assert (want[0], want[1], True) in dots
        assert P.dset_key(2, 1023, (1 << 48) - 2) < P.TOP  # the largest packed key is not KF_EMPTY


def test_probe_wraps_the_table_end():
    st, ds, dots = P.dot_edges("probe wrap")
    for reverse in (False, True):  # whichever of the two dots arrives second sits past the end
        tab = P.dset_table(ds, reverse)
        assert len(tab) == 1024 and sum(x is not None for x in tab) <= 512
        wraps = 0
        for node, cnt, in_ctx in dots:
            found, seen = P.dset_probe(tab, P.WRAP_DELTA, node, cnt)
            assert found == in_ctx and seen[0] == 1023
            wraps += len(seen) > 1 and seen[1] == 0
        assert wraps >= 2  # one of the dots held, and the absent one


# ---------------------------------------------------------------- reach: two passes, hygiene

def test_two_pass_reach():
    a, b = P.traces(*P.two_pass("second prep fails"))
    assert a["verdict"] == "first" and b["verdict"] == "refuse" and b["host"] is not None
    a, b = P.traces(*P.two_pass("second overflows twice"))
    assert a["verdict"] == "first" and b["verdict"] == "refuse" and b["host"] is None
    assert all(x["first"] == [0] for x in b["attempts"])
    a, b = P.traces(*P.two_pass("first retries"))
    assert a["verdict"] == "retry" and b["verdict"] == "first"
    assert len(a["attempts"][0]["first"]) == 1 and not a["attempts"][1]["first"]
    st, ds = P.two_pass("first retries")
    assert len(ds) == 70 and P.plan(st, ds[:64], a["T0"])[a["attempts"][0]["first"][0]]["why"] in ("M", "UM")
    assert P.verdict(st, ds) == "retry"


def test_hygiene_inputs_reach():
    """The two flagged calls of the hygiene test: KF_PREP_FAIL (no ticket taken) and
    KF_OVERFLOW twice (every ticket taken, bucket 0 over at both T)."""
    prep, over = P.hygiene_inputs()
    assert P.trace_pass(*prep)["host"] == "node >= KNT in the state's context"
    tr = P.trace_pass(*over)
    assert tr["verdict"] == "refuse" and tr["host"] is None
    assert [a["first"] for a in tr["attempts"]] == [[0], [0]]
    assert P.verdict(*random_fold(0, n_keys=3000, k=1)) == "first"
    assert P.verdict(*P.at_capacity("keep", True, "many")) == "retry"


# ---------------------------------------------------------------- the inputs are stores

def all_inputs():
    for layout in ("one", "many"):
        for spread in (False, True):
            for over in (None,) + P.OVERS:
                yield f"at_capacity {over} {spread} {layout}", *P.at_capacity(over, spread, layout)
    for name in P.SKEW_CASES:
        yield name, *P.skew_case(name)
    for f in (P.one_sub_bucket, P.one_key_bucket, P.ends, P.all_runs_one_bucket, P.gaps,
              P.tiny_absent_keys):
        yield f.__name__, *f()
    for case in P.DOT_CASES:
        yield case, *P.dot_edges(case)[:2]
    for case in ("second prep fails", "second overflows twice", "first retries"):
        yield case, *P.two_pass(case)


def test_every_generator_gives_stores():
    """Sorted rows, distinct tuples, unique dots (ref_store_check); keysets sorted and unique;
    contexts sorted by (node, counter) without repeats; nothing above ~10k rows or 70 deltas."""
    n = 0
    for name, st, ds in all_inputs():
        n += 1
        assert len(st["rows"][0]) <= 10_000 and len(ds) <= 70, name
        assert R.store_check(st["rows"]), name
        for d in ds:
            assert R.store_check(d["rows"]), name
            if d["keys"] is not None:
                assert d["keys"].dtype == np.uint64 and bool(np.all(d["keys"][1:] > d["keys"][:-1])), name
        for kind, node, cnt in [st["ctx"]] + [d["ctx"] for d in ds]:
            assert node.dtype == np.uint32 and cnt.dtype == np.uint64, name
            order = list(zip(node.tolist(), cnt.tolist()))
            assert order == sorted(set(order)), name
            if kind != DOTS:
                assert len(set(node.tolist())) == len(node), name
    assert n == 20 + len(P.SKEW_CASES) + 6 + 5 + 3


# ---------------------------------------------------------------- the reference on these shapes

def term_fold(st, ds):
    t = soa_to_term(st["rows"], st["ctx"])
    for d in ds:
        dt = soa_to_term(d["rows"], d["ctx"])
        ks = sorted(set(t.value) | set(dt.value)) if d["keys"] is None else [int(x) for x in d["keys"]]
        t = T.join(t, dt, ks)
    return term_to_soa_raw(t)


SMALL = {
    "at_capacity one": lambda: P.at_capacity(),
    "at_capacity many": lambda: P.at_capacity(layout="many"),
    "at_capacity keep many": lambda: P.at_capacity("keep", True, "many"),
    "at_capacity S one": lambda: P.at_capacity("S", False, "one"),
    "one_key_bucket": P.one_key_bucket,
    "ends": P.ends,
    "all_runs_one_bucket": P.all_runs_one_bucket,
    "tiny_absent_keys": P.tiny_absent_keys,
    **{"dots " + c: (lambda c=c: P.dot_edges(c)[:2]) for c in P.DOT_CASES},
}


@pytest.mark.parametrize("name", list(SMALL))
def test_c_oracle_equals_term_oracle_on(name):
    """R.apply_deltas (what the GPU tests compare with) == the term-level fold of join/3 on the
    new generators' shapes, as tests/test_configs.py pins it on random_fold."""
    st, ds = SMALL[name]()
    rows, ctx = R.apply_deltas(st["rows"], st["ctx"], [d["rows"] for d in ds],
                               [d["ctx"] for d in ds], [d["keys"] for d in ds])
    wrows, wctx = term_fold(st, ds)
    assert rows_equal(rows, wrows) and ctx_equal(ctx, wctx)
    assert 0 < len(rows[0])
    if name.startswith("dots "):
        # the extra rows: removed exactly when delta 1's context holds their dot
        _, _, dots = P.dot_edges(name[5:])
        for node, cnt, in_ctx in dots:
            alive = bool(np.any((rows[3] == node) & (rows[4] == np.uint64(cnt))))
            assert alive == (not in_ctx), (node, cnt)
