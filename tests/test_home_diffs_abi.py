"""dg_join_delta_home_diffs and the replica layer's *_diffs calls at their C boundaries,
without a GPU: the header declares and the library exports the entry point, the four
DG_HOME_DIFF* macros are what gcc computes and lay the three ranges out behind the plain
block, replica.h's two functions and dgr_diffs match the ctypes mirror in nif.py, the ABI
version is still 4, and a null `home` is refused before any device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "replica.h"
int main(void) {
  printf("%d %d %d %d %d %d\n", (int)DG_HOME_WORDS, (int)DG_HOME_DIFF_OLD, (int)DG_HOME_DIFF_NEW,
         (int)DG_HOME_DIFF_FLAGS, (int)DG_HOME_DIFFS_WORDS, DG_ABI_VERSION);
  printf("%zu %zu %zu %zu %zu\n", sizeof(dgr_diffs), offsetof(dgr_diffs, n), offsetof(dgr_diffs, old_val),
         offsetof(dgr_diffs, new_val), offsetof(dgr_diffs, flags));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("home_diffs")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "c_src"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return [[int(x) for x in line.split()] for line in out]


def test_header_library_and_mirror_have_the_entry_point(lib):
    assert "dg_join_delta_home_diffs" in _abi.header_functions()
    assert hasattr(lib, "dg_join_delta_home_diffs")
    # exactly dg_join_delta_home's arguments
    assert _abi._SIGS["dg_join_delta_home_diffs"] == _abi._SIGS["dg_join_delta_home"]
    assert lib.dg_abi_version() == 4


def test_macros_are_the_layout(layout):
    words, old, new, flags, total, abi = layout[0]
    assert abi == 4
    assert [words, old, new, flags, total] == [_abi.DG_HOME_WORDS, _abi.DG_HOME_DIFF_OLD, _abi.DG_HOME_DIFF_NEW,
                                               _abi.DG_HOME_DIFF_FLAGS, _abi.DG_HOME_DIFFS_WORDS]
    # behind the plain block: 512 old ids, 512 new ids, 512 flag BYTES
    assert old == words and new == old + 512 and flags == new + 512 and total == flags + 512 // 8


def test_replica_header_declares_the_diffs_calls(layout):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "c_src", "replica.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dgr_[a-z_]+)\s*\(([^;]*)\)\s*;", text)}
    for name, plain in (("dgr_join_delta_diffs", "dgr_join_delta"), ("dgr_mutate_batch_diffs", "dgr_mutate_batch")):
        assert name in decl and name in nif._SIGS
        # the plain call's parameters, then `dgr_diffs* diffs`
        params = [p.strip() for p in decl[name].split(",")]
        assert params[:-1] == [p.strip() for p in decl[plain].split(",")]
        assert re.fullmatch(r"dgr_diffs\s*\*\s*diffs", params[-1])
        res, args = nif._SIGS[name]
        pres, pargs = nif._SIGS[plain]
        assert res is pres and args[:-1] == pargs and args[-1] is C.POINTER(nif.dgr_diffs)
        assert len(args) == len(params)
    D = nif.dgr_diffs
    assert layout[1] == [C.sizeof(D), D.n.offset, D.old_val.offset, D.new_val.offset, D.flags.offset]


def test_replica_library_exports_the_diffs_calls(lib):
    r = nif.load()
    assert hasattr(r, "dgr_join_delta_diffs") and hasattr(r, "dgr_mutate_batch_diffs")
    # a null state or a null diffs is refused before anything is looked at
    ch, df = nif.dgr_changed(), nif.dgr_diffs()
    s, x = _abi.dg_store(), _abi.dg_context()
    assert r.dgr_join_delta_diffs(None, 1, C.byref(s), C.byref(x), None, 0, C.byref(ch),
                                  C.byref(df)) == _abi.DG_E_INVAL
    assert r.dgr_mutate_batch_diffs(None, 1, 0, 0, None, None, None, None, C.byref(ch),
                                    C.byref(df)) == _abi.DG_E_INVAL


def test_null_home_is_refused_before_any_device_call(lib):
    s, x = _abi.dg_store(), _abi.dg_context()
    sw = C.c_int(7)
    eng = C.c_void_p(1)  # never dereferenced: the null check comes first
    for f in (lib.dg_join_delta_home_diffs, lib.dg_join_delta_home):
        assert f(eng, C.byref(s), C.byref(x), C.byref(s), C.byref(x), None, 0, C.byref(s), None, None,
                 C.byref(sw)) == _abi.DG_E_INVAL
        assert b"null argument" in lib.dg_last_error()
    assert lib.dg_join_delta_home_diffs(None, C.byref(s), C.byref(x), C.byref(s), C.byref(x), None, 0,
                                        C.byref(s), None, None, C.byref(sw)) == _abi.DG_E_INVAL
