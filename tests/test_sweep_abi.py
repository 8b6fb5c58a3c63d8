"""dg_mark_ids / dgr_sweep / dgm_sweep_* at the library boundaries, without a GPU: the
libraries export them, the ctypes signature tables carry them, and dg_mark_ids validates its
arguments before any device call (so the answers are the same on a machine without a GPU)."""
import ctypes as C
import os

import pytest

from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_libraries_export_the_sweep_functions(lib):
    assert "dg_mark_ids" in _abi.header_functions()
    assert hasattr(lib, "dg_mark_ids")
    marshal = C.CDLL(os.path.join(ROOT, "c_src", "_build", "libdgmarshal.so"))
    for name in ("dgm_sweep_values", "dgm_sweep_keys", "dgm_key_ids_sorted", "dgm_key_count"):
        assert hasattr(marshal, name), name
    replica = C.CDLL(os.path.join(ROOT, "c_src", "_build", "libdgreplica.so"))
    assert hasattr(replica, "dgr_sweep")


def test_signature_tables_carry_them():
    res, args = _abi._SIGS["dg_mark_ids"]
    assert res is C.c_int and len(args) == 9
    res, args = nif._SIGS["dgr_sweep"]
    assert res is C.c_int and len(args) == 7
    assert (_abi.DG_COL_KEY, _abi.DG_COL_VAL) == (0, 1)


def test_mark_ids_rejects_bad_arguments_before_any_device_call(lib):
    s = (_abi.dg_store * 1)()
    n, x = C.c_uint64(), C.c_uint64()
    ids = (C.c_uint64 * 4)(1, 2, 3, 4)
    used = (C.c_uint8 * 4)()
    idp = C.cast(ids, _abi.P64)
    # a NULL engine
    assert lib.dg_mark_ids(None, s, 1, _abi.DG_COL_VAL, idp, 4, used, C.byref(n), C.byref(x)) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    # a column that is neither key nor value
    for col in (2, -1):
        assert lib.dg_mark_ids(None, s, 1, col, idp, 4, used, C.byref(n), C.byref(x)) == _abi.DG_E_INVAL
        assert b"bad column" in lib.dg_last_error()
    # NULL flags (or a NULL table) with n_ids > 0
    assert lib.dg_mark_ids(None, s, 1, _abi.DG_COL_KEY, idp, 4, None, C.byref(n), C.byref(x)) == _abi.DG_E_INVAL
    assert b"null id table or flags" in lib.dg_last_error()
    assert lib.dg_mark_ids(None, s, 1, _abi.DG_COL_KEY, None, 4, used, C.byref(n), C.byref(x)) == _abi.DG_E_INVAL
    assert b"null id table or flags" in lib.dg_last_error()
    # NULL stores with n_stores > 0, a NULL count
    assert lib.dg_mark_ids(None, None, 2, _abi.DG_COL_KEY, idp, 4, used, C.byref(n), C.byref(x)) == _abi.DG_E_INVAL
    assert b"null stores" in lib.dg_last_error()
    assert lib.dg_mark_ids(None, s, 1, _abi.DG_COL_KEY, idp, 4, used, None, None) == _abi.DG_E_INVAL
    assert b"null n_used" in lib.dg_last_error()


def test_abi_version_is_unchanged(lib):
    assert lib.dg_abi_version() == 4
