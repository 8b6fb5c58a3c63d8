"""dg_lww_diffs at the C-ABI boundary without a GPU: the ctypes mirror matches gcc's layout
of the header's struct, both entry points are exported and validate their arguments before
any device call, and the expected-diffs helper of the GPU tests (lww_diffs_cases.py) is
pinned by known answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.build import build
from lww_diffs_cases import NEW, OLD, classes, expected_diffs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "deltagpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d %d %d\n", sizeof(dg_lww_diffs), offsetof(dg_lww_diffs, old_val),
         offsetof(dg_lww_diffs, new_val), offsetof(dg_lww_diffs, flags), offsetof(dg_lww_diffs, cap),
         DG_DIFF_OLD, DG_DIFF_NEW, DG_ABI_VERSION);
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_struct_layout_matches_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _abi.dg_lww_diffs
    assert got == [C.sizeof(D), D.old_val.offset, D.new_val.offset, D.flags.offset, D.cap.offset,
                   _abi.DG_DIFF_OLD, _abi.DG_DIFF_NEW, 4]
    assert (OLD, NEW) == (_abi.DG_DIFF_OLD, _abi.DG_DIFF_NEW)


def test_entry_points_are_exported_and_reject_bad_arguments(lib):
    """Validation comes before any device call, so it is the same without a GPU."""
    assert {"dg_read_diff", "dg_join_delta_diffs"} <= set(_abi.header_functions())
    s, x, d = _abi.dg_store(), _abi.dg_context(), _abi.dg_lww_diffs()
    n, sw = C.c_uint64(), C.c_int()
    assert lib.dg_read_diff(None, C.byref(s), C.byref(s), None, 0, C.byref(d)) == _abi.DG_E_INVAL
    # no diffs, and diffs->cap < cap: DG_E_INVAL before the engine is even looked at
    args = (None, C.byref(s), C.byref(x), C.byref(s), C.byref(x), None, 0, C.byref(s), None, None, 8,
            C.byref(n), C.byref(sw), None, None)
    assert lib.dg_join_delta_diffs(*args, None) == _abi.DG_E_INVAL
    d.cap = 7
    assert lib.dg_join_delta_diffs(*args, C.byref(d)) == _abi.DG_E_INVAL
    assert b"diffs cap 7 < changed cap 8" in lib.dg_last_error()


def _rows(r):
    a = np.array(sorted(r), dtype=np.int64).reshape(-1, 5)
    return (a[:, 0].astype(np.uint64), a[:, 1].astype(np.uint64), a[:, 2].copy(), a[:, 3].astype(np.uint32),
            a[:, 4].astype(np.uint64))


def test_expected_diffs_known_answers():
    """read/1 keeps the FIRST entry of maximal ts in ({val, ts}) order (aw_lww_map.ex:211-216,
    SURVEY H2): on a tie at the maximal ts the smallest value wins."""
    #        key val ts node cnt
    old = _rows([(10, 5, 9, 0, 1), (10, 3, 9, 1, 1), (10, 7, 2, 0, 2),   # tie at ts 9: 3 wins
                 (20, 4, 1, 0, 3),                                      # removed below
                 (30, 8, -5, 0, 4), (30, 2, -7, 1, 2),                   # negative ts: 8 (ts -5) wins
                 (50, 6, 4, 0, 5)])
    new = _rows([(10, 5, 9, 0, 1), (10, 3, 9, 1, 1), (10, 1, 8, 2, 1),   # still 3 (1 has a smaller ts)
                 (30, 8, -5, 0, 4), (30, 9, -5, 2, 2),                   # tie at -5: 8 stays
                 (40, 2, 0, 2, 3),                                      # added
                 (50, 6, 4, 0, 5), (50, 1, 6, 2, 4)])                    # updated: ts 6 wins
    keys = np.array([50, 10, 20, 99, 30, 40, 10], np.uint64)            # any order, a repeat, an absent key
    ov, nv, fl = expected_diffs(old, new, keys)
    assert ov.tolist() == [6, 3, 4, 0, 8, 0, 3]
    assert nv.tolist() == [1, 3, 0, 0, 8, 2, 3]
    assert fl.tolist() == [3, 3, OLD, 0, 3, NEW, 3]
    u = np.array([10, 20, 30, 40, 50], np.uint64)
    assert classes(new, u, *expected_diffs(old, new, u)) == {
        "unchanged": 2, "removed": 1, "added": 1, "updated": 1, "ties": 2}
    # an empty side reads nothing
    none = tuple(c[:0] for c in old)
    ov, nv, fl = expected_diffs(none, new, u)
    assert ov.tolist() == [0] * 5 and fl.tolist() == [NEW, 0, NEW, NEW, NEW]
