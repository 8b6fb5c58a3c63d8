"""dg_merkle_diff_take at its boundary without a GPU: the prototype compiles from the header with
gcc and fails with an argument dropped, the ctypes signature matches, the library exports it, the
ABI version is still 4, every DG_E_INVAL case is rejected before any device call (a fake engine
that is never used), the scratch layout (csrc/dg_diff_scratch.h) holds under ASan and UBSan in a
stand-alone program, and each case of diff_take_cases.py takes the path it is named for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diff_take_cases as D
from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build
from oracle import ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include")]
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")

PROTO_C = r"""
#include "deltagpu.h"
typedef int (*diff_take_fn)(dg_engine*, const dg_merkle*, const dg_store*, const dg_merkle*, const dg_store*, int,
                            uint64_t*, uint64_t, uint64_t*, dg_store*, uint64_t*, uint64_t*);
diff_take_fn f = dg_merkle_diff_take;
_Static_assert(DG_ABI_VERSION == 4, "the addition is additive");
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_prototype_compiles_and_the_signature_matches(tmp_path, lib):
    src = tmp_path / "proto.c"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(src), "-o", str(tmp_path / "proto.o")], check=True)
    bad = tmp_path / "bad.c"
    bad.write_text(PROTO_C.replace("const dg_store*, int,", "const dg_store*,"))
    assert subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(bad), "-o", str(tmp_path / "bad.o")],
                          capture_output=True).returncode != 0
    assert lib.dg_abi_version() == 4
    assert "dg_merkle_diff_take" in set(_abi.header_functions())
    S, M, P = C.POINTER(_abi.dg_store), C.POINTER(_abi.dg_merkle), _abi.P64
    sig = _abi._SIGS["dg_merkle_diff_take"]
    assert sig == (C.c_int, [C.c_void_p, M, S, M, S, C.c_int, P, C.c_uint64, P, S, P, P])
    assert lib.dg_merkle_diff_take.argtypes == sig[1]  # (the library exports it)
    # dg_merkle_diff's own signature is untouched
    assert _abi._SIGS["dg_merkle_diff"] == (C.c_int, [C.c_void_p, M, S, M, S, P, C.c_uint64, P, P])


def _tree(depth=8):
    """a tree that passes the shape checks (its arrays are never read before a launch)"""
    t = _abi.dg_merkle()
    t.depth = depth
    t.nodes = 64
    t.counts = 64
    return t


def test_the_call_rejects_bad_arguments_before_any_launch(lib):
    ta, tb, s = _tree(), _tree(), _abi.dg_store()
    fake = C.c_void_p(1)
    words = (C.c_uint64 * 16)()
    p = C.cast(words, C.c_void_p)
    p64 = C.cast(words, _abi.P64)
    n, tot = C.c_uint64(), C.c_uint64()
    good = lambda: _abi.dg_store(p, p, p, p, p, 0, 2)

    def call(e=fake, a=ta, b=tb, side=1, out=p64, cap=4, offs=p64, rows=None, n_out=C.byref(n)):
        rows = C.byref(good()) if rows is None else rows
        return lib.dg_merkle_diff_take(e, C.byref(a), C.byref(s), C.byref(b), C.byref(s), side, out, cap, offs, rows,
                                       n_out, C.byref(tot))

    assert call(e=None) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    assert call(n_out=None) == _abi.DG_E_INVAL
    assert b"dg_merkle_diff_take: null n_out" in lib.dg_last_error()
    assert call(out=None) == _abi.DG_E_INVAL
    assert b"null out_keys" in lib.dg_last_error()
    assert call(offs=None) == _abi.DG_E_INVAL
    assert b"null offs" in lib.dg_last_error()
    null_rows = C.POINTER(_abi.dg_store)()
    assert call(rows=null_rows) == _abi.DG_E_INVAL
    assert b"null rows" in lib.dg_last_error()
    for col in ("key", "val", "ts", "node", "cnt"):
        r = good()
        setattr(r, col, None)
        assert call(rows=C.byref(r)) == _abi.DG_E_INVAL
        assert b"null column with cap=2" in lib.dg_last_error()
    for side in (-1, 2, 77):
        assert call(side=side) == _abi.DG_E_INVAL
        assert b"side" in lib.dg_last_error()
    # the tree shape checks are dg_merkle_diff's
    assert call(b=_tree(9)) == _abi.DG_E_INVAL
    assert b"dg_merkle_diff_take: trees of different shape" in lib.dg_last_error()
    sharded = _tree()
    sharded.shard_bits, sharded.shard = 1, 1
    assert call(b=sharded) == _abi.DG_E_INVAL
    assert b"trees of different shape" in lib.dg_last_error()


REPLICA_PROTO_C = r"""
#include "replica.h"
typedef int (*sync_fn)(dgr_state*, uint64_t, dgr_state*, uint64_t, uint64_t, dgr_changed*, uint64_t*);
sync_fn f = dgr_sync_from;
typedef int (*sync_diffs_fn)(dgr_state*, uint64_t, dgr_state*, uint64_t, uint64_t, dgr_changed*, dgr_diffs*,
                             uint64_t*);
sync_diffs_fn g = dgr_sync_from_diffs;
"""


@pytest.fixture(scope="module")
def rlib(lib):
    if not os.path.exists(nif.LIB_PATH) or not hasattr(C.CDLL(nif.LIB_PATH), "dgr_sync_from"):
        R.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    return nif.load()


def test_the_replica_prototypes_compile_and_the_signatures_match(tmp_path, rlib):
    inc = [*INC, "-I", os.path.join(ROOT, "c_src")]
    src = tmp_path / "rproto.c"
    src.write_text(REPLICA_PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *inc, "-c", str(src), "-o", str(tmp_path / "rproto.o")], check=True)
    for drop in ("uint64_t, dgr_changed*, uint64_t*);", "dgr_changed*, dgr_diffs*,"):
        bad = tmp_path / "rbad.c"
        assert drop in REPLICA_PROTO_C
        bad.write_text(REPLICA_PROTO_C.replace(drop, drop.replace("dgr_changed*, ", "")))
        assert subprocess.run(["gcc", "-Wall", "-Werror", *inc, "-c", str(bad), "-o", str(tmp_path / "rbad.o")],
                              capture_output=True).returncode != 0
    VP, U64, PU64 = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert nif._SIGS["dgr_sync_from"] == (C.c_int32, [VP, U64, VP, U64, U64, C.POINTER(nif.dgr_changed), PU64])
    assert nif._SIGS["dgr_sync_from_diffs"] == (C.c_int32, [VP, U64, VP, U64, U64, C.POINTER(nif.dgr_changed),
                                                            C.POINTER(nif.dgr_diffs), PU64])
    assert rlib.dgr_sync_from.argtypes == nif._SIGS["dgr_sync_from"][1]  # (the library exports them)
    assert rlib.dgr_sync_from_diffs.argtypes == nif._SIGS["dgr_sync_from_diffs"][1]


def test_the_replica_call_rejects_bad_arguments_before_any_launch(rlib):
    """Null arguments, dst == src, states of different engines and states without a tree, with
    fake states that are never used: zeroed blocks whose first word (the engine) is set."""
    def fake_state(engine_word):
        blk = (C.c_uint64 * 512)()
        blk[0] = engine_word
        return blk

    a, b, other = fake_state(0x1000), fake_state(0x1000), fake_state(0x2000)
    pa, pb, po = (C.cast(x, C.c_void_p) for x in (a, b, other))
    ch, df, tot = nif.dgr_changed(), nif.dgr_diffs(), C.c_uint64()
    f, fd = rlib.dgr_sync_from, rlib.dgr_sync_from_diffs
    E = _abi.DG_E_INVAL
    assert f(None, 0, pb, 0, 0, C.byref(ch), C.byref(tot)) == E
    assert f(pa, 0, None, 0, 0, C.byref(ch), C.byref(tot)) == E
    assert f(pa, 0, pb, 0, 0, None, C.byref(tot)) == E
    assert f(pa, 0, pb, 0, 0, C.byref(ch), None) == E
    assert fd(pa, 0, pb, 0, 0, C.byref(ch), None, C.byref(tot)) == E
    assert f(pa, 0, pa, 0, 0, C.byref(ch), C.byref(tot)) == E      # dst == src
    assert f(pa, 0, po, 0, 0, C.byref(ch), C.byref(tot)) == E      # different engines
    assert f(pa, 0, pb, 0, 0, C.byref(ch), C.byref(tot)) == E      # one engine, no trees
    assert fd(pa, 0, pb, 0, 5, C.byref(ch), C.byref(df), C.byref(tot)) == E


def test_scratch_layout_under_sanitizers(tmp_path):
    """tests/diff_take_layout.cc: the diff's arrays stay where they are, the take's two arrays
    follow, disjoint and inside the block, and the whole grows by na + nb + 1 + tiles words."""
    exe = str(tmp_path / "diff_take_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "diff_take_layout.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "2450 regions checked, 0 failures" in r.stdout, r.stdout[-2000:]


def test_the_model_restates_the_kernels_capacities():
    text = open(os.path.join(CSRC, "merkle_diff.hip")).read()
    assert "constexpr u32 RCAP = XSUB >= 4096 ? 1664 : 640;" in text
    assert "constexpr u32 DCAP = XSUB >= 4096 ? 512 : 160;" in text
    assert "#define DG_DIFF_SUB 12" in open(os.path.join(CSRC, "dg_diff_scratch.h")).read()
    assert (D.RCAP, D.DCAP, D.SUB) == (1664, 512, 12)


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_each_case_takes_the_path_it_is_named_for(case):
    a, b = D.pair(case)
    f = D.figures(a, b, case.depth)
    paths = {D.lds_path(r, n) for r, n in zip(f.R, f.ND)}
    assert paths == {case.path == "lds"}, (f.R, f.ND)  # every differing subtree
    if case.fullest:
        assert D.fullest(f) == case.fullest
    runs = lambda rows: int(np.unique(rows[0], return_counts=True)[1].max())
    if case.name == "random300_d12":
        d = R.store_diff(a, b)
        assert int((~np.isin(d, b[0])).sum()) == 22 and int((~np.isin(d, a[0])).sum()) == 59  # only in A / only in B
        assert max(runs(a), runs(b)) == 5
    if case.name == "random300_d8":
        assert f.subtrees == 1  # a 256-bucket subtree: the per-thread node-load branch
    if case.name == "random3000_d14":
        assert f.subtrees == 4 and len(f.differing) == 4
    if case.name == "random3000_d5":
        assert f.subtrees == 1 and D.fullest(f)[1] == 32  # a 32-bucket tree: two threads own all of it
    if case.name == "merkle20000_d21":
        assert f.subtrees == 512 and len(f.differing) == 444  # two groups of 256 subtrees
        assert min(f.differing) < 256 <= max(f.differing)
    if case.name.startswith("hot"):
        assert max(runs(a), runs(b)) == 200  # past the 127 a run-length byte holds: the "longer" branch

