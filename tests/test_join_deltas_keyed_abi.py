"""dg_join_deltas_keyed at the C-ABI boundary without a GPU: its prototype compiles from the
header with gcc and takes the arguments _abi.py declares, it is exported, DG_KEYED_FALLBACK is
the header's, the ABI version is still 4, and the arguments are validated -- and a batch the
host can tell is not served is declined -- before any device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTO_C = r"""
#include "deltagpu.h"
typedef int (*keyed_fn)(dg_engine*, dg_store*, dg_context*, int, const dg_store*, const dg_context*,
                        const uint64_t* const*, const uint64_t*, dg_store*, dg_merkle*, uint64_t*,
                        uint64_t, uint64_t*, dg_store*, dg_context*, dg_lww_diffs*, int*);
keyed_fn g = dg_join_deltas_keyed;
_Static_assert(DG_ABI_VERSION == 4, "the addition is additive");
_Static_assert(DG_KEYED_FALLBACK > 0, "a positive code: not an error");
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_prototype_compiles_and_matches_the_ctypes_view(tmp_path, lib):
    src, obj = tmp_path / "proto.c", tmp_path / "proto.o"
    src.write_text(PROTO_C)
    cmd = ["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c"]
    subprocess.run(cmd + [str(src), "-o", str(obj)], check=True)
    bad = tmp_path / "bad.c"  # without `swapped` it does not compile (the check can fail)
    bad.write_text(PROTO_C.replace("dg_lww_diffs*, int*);", "dg_lww_diffs*);"))
    assert subprocess.run(cmd + [str(bad), "-o", str(obj)], capture_output=True).returncode != 0
    assert _abi._SIGS["dg_join_deltas_keyed"] == (_abi._SIGS["dg_join_deltas"][0],
                                                  _abi._SIGS["dg_join_deltas"][1] + [C.POINTER(C.c_int)])
    assert lib.dg_join_deltas_keyed.argtypes == _abi._SIGS["dg_join_deltas_keyed"][1]
    header = open(_abi.HEADER).read()
    assert int(re.search(r"#define DG_KEYED_FALLBACK (\d+)", header).group(1)) == _abi.DG_KEYED_FALLBACK
    assert lib.dg_abi_version() == 4


def test_exported_validates_and_declines_before_any_device_call(lib):
    assert "dg_join_deltas_keyed" in _abi.header_functions()
    s, x = _abi.dg_store(), _abi.dg_context()
    n, sw = C.c_uint64(7), C.c_int(5)
    keep = (C.c_uint64 * 8)()
    kp, nk = (C.c_void_p * 1)(), (C.c_uint64 * 1)(0)
    fake = C.c_void_p(1)  # an engine-shaped pointer: the checks below run before it is used

    def call(e, k, deltas, keys, nks, swapped=sw, state_ctx=x):
        return lib.dg_join_deltas_keyed(e, C.byref(s), C.byref(state_ctx), k, deltas,
                                        None if deltas is None else C.byref(x), keys, nks, C.byref(s), None, keep, 8,
                                        C.byref(n), None, None, None, None if swapped is None else C.byref(swapped))
    assert call(None, 0, None, None, None) == _abi.DG_E_INVAL and b"null engine" in lib.dg_last_error()
    assert call(fake, 1, C.byref(s), kp, nk, swapped=None) == _abi.DG_E_INVAL
    assert b"null swapped" in lib.dg_last_error()
    assert call(fake, -1, None, None, None) == _abi.DG_E_INVAL
    assert call(fake, 1, C.byref(s), kp, None) == _abi.DG_E_INVAL and b"keys without n_keys" in lib.dg_last_error()
    big = _abi.dg_store(8, 8, 8, 8, 8, 5, 5)
    assert call(fake, 1, C.byref(big), kp, nk) == _abi.DG_E_CAPACITY
    assert b"dg_join_deltas_keyed: spare cap 0 < 5 rows in" in lib.dg_last_error()
    # declined on the host: no keysets at all, a NULL keyset, a dot-set state context
    assert call(fake, 1, C.byref(s), None, None) == _abi.DG_KEYED_FALLBACK
    assert call(fake, 1, C.byref(s), kp, nk) == _abi.DG_KEYED_FALLBACK
    dots = _abi.dg_context()
    dots.kind = _abi.DG_CTX_DOTS
    kp[0] = 8
    assert call(fake, 1, C.byref(s), kp, nk, state_ctx=dots) == _abi.DG_KEYED_FALLBACK
    assert n.value == 0 and sw.value == 0
