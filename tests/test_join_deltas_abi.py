"""dg_store_diff and dg_join_deltas at the C-ABI boundary without a GPU: their prototypes
compile from the header with gcc and take the arguments _abi.py declares, both are exported,
the ABI version is still 4, and they validate their arguments before any device call."""
import ctypes as C
import os
import subprocess

import pytest

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Assigning each function to a pointer of the expected type fails to compile (-Werror) when
# the header's prototype differs; the program prints the argument counts and the version.
PROTO_C = r"""
#include <stdio.h>
#include "deltagpu.h"
typedef int (*store_diff_fn)(dg_engine*, const dg_store*, const dg_store*, uint64_t*, uint64_t, uint64_t*,
                             dg_store*, dg_lww_diffs*);
typedef int (*join_deltas_fn)(dg_engine*, dg_store*, dg_context*, int, const dg_store*, const dg_context*,
                              const uint64_t* const*, const uint64_t*, dg_store*, dg_merkle*, uint64_t*,
                              uint64_t, uint64_t*, dg_store*, dg_context*, dg_lww_diffs*);
store_diff_fn f = dg_store_diff;
join_deltas_fn g = dg_join_deltas;
_Static_assert(DG_ABI_VERSION == 4, "the additions are additive");
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_prototypes_compile_and_match_the_ctypes_view(tmp_path, lib):
    src, obj = tmp_path / "proto.c", tmp_path / "proto.o"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(obj)], check=True)
    # ... and a prototype with one argument fewer does not (the check can fail)
    bad = tmp_path / "bad.c"
    bad.write_text(PROTO_C.replace("uint64_t*,\n                             dg_store*, dg_lww_diffs*);",
                                   "uint64_t*,\n                             dg_store*);"))
    assert subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(bad),
                           "-o", str(obj)], capture_output=True).returncode != 0
    n_diff, n_join = 8, 16  # the arguments of the two function pointer types above
    assert lib.dg_abi_version() == 4
    P = C.POINTER
    S, X, D = P(_abi.dg_store), P(_abi.dg_context), P(_abi.dg_lww_diffs)
    assert _abi._SIGS["dg_store_diff"] == (C.c_int, [C.c_void_p, S, S, _abi.P64, C.c_uint64, _abi.P64, S, D])
    assert _abi._SIGS["dg_join_deltas"] == (C.c_int, [C.c_void_p, S, X, C.c_int, S, X, P(C.c_void_p), _abi.P64,
                                                      S, C.c_void_p, _abi.P64, C.c_uint64, _abi.P64, S, X, D])
    assert len(_abi._SIGS["dg_store_diff"][1]) == n_diff and len(_abi._SIGS["dg_join_deltas"][1]) == n_join
    assert lib.dg_store_diff.argtypes == _abi._SIGS["dg_store_diff"][1]
    assert lib.dg_join_deltas.argtypes == _abi._SIGS["dg_join_deltas"][1]


def test_entry_points_are_exported_and_reject_bad_arguments(lib):
    """Validation comes before any device call, so it is the same without a GPU."""
    assert {"dg_store_diff", "dg_join_deltas"} <= set(_abi.header_functions())
    s, x, d = _abi.dg_store(), _abi.dg_context(), _abi.dg_lww_diffs()
    n = C.c_uint64(7)
    assert lib.dg_store_diff(None, C.byref(s), C.byref(s), None, 0, C.byref(n), None, None) == _abi.DG_E_INVAL
    assert lib.dg_join_deltas(None, C.byref(s), C.byref(x), 0, None, None, None, None, C.byref(s), None, None, 0,
                              C.byref(n), None, None, None) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    # with an engine-shaped pointer the argument checks run before the engine is used
    fake = C.c_void_p(1)
    assert lib.dg_store_diff(fake, C.byref(s), C.byref(s), None, 8, C.byref(n), None, None) == _abi.DG_E_INVAL
    d.cap = 7
    keep = (C.c_uint64 * 8)()
    assert lib.dg_store_diff(fake, C.byref(s), C.byref(s), keep, 8, C.byref(n), None, C.byref(d)) == _abi.DG_E_INVAL
    assert b"diffs cap 7 < changed cap 8" in lib.dg_last_error() and n.value == 0
    # k < 0, deltas missing, keys without their counts
    args = lambda k, deltas, keys, nk: (fake, C.byref(s), C.byref(x), k, deltas, None if deltas is None else C.byref(x),
                                        keys, nk, C.byref(s), None, keep, 8, C.byref(n), None, None, None)
    kp = (C.c_void_p * 1)()
    assert lib.dg_join_deltas(*args(-1, None, None, None)) == _abi.DG_E_INVAL
    assert lib.dg_join_deltas(*args(1, None, None, None)) == _abi.DG_E_INVAL
    assert lib.dg_join_deltas(*args(1, C.byref(s), kp, None)) == _abi.DG_E_INVAL
    assert b"keys without n_keys" in lib.dg_last_error()
    # capacities: a spare and a context too small for the sums, before anything is touched
    big = _abi.dg_store(8, 8, 8, 8, 8, 5, 5)
    nk = (C.c_uint64 * 1)(0)
    assert lib.dg_join_deltas(fake, C.byref(s), C.byref(x), 1, C.byref(big), C.byref(x), kp, nk, C.byref(s), None,
                              keep, 8, C.byref(n), None, None, None) == _abi.DG_E_CAPACITY
    assert b"spare cap 0 < 5 rows in" in lib.dg_last_error()
