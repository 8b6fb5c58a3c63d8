"""dg_take_keysets and dgr_take_batch at their boundaries without a GPU: the prototypes compile
from the headers with gcc and take the arguments the ctypes tables declare, the libraries
export them and the pack helpers, dgr_taken is laid out in nif.py as the C compiler lays it
out, the ABI version is still 4, and null arguments are rejected before any device call."""
import ctypes as C
import os
import subprocess

import pytest

from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "c_src")]

# Assigning each function to a pointer of the expected type fails to compile (-Werror) when
# the header's prototype differs.
PROTO_C = r"""
#include "replica.h"
typedef int (*take_keysets_fn)(dg_engine*, const dg_store*, int, const uint64_t* const*, const uint64_t*,
                               uint64_t*, uint64_t*, uint64_t*, uint64_t, uint64_t*, dg_store*);
typedef int (*take_batch_fn)(dgr_state*, uint64_t, int, const uint64_t* const*, const uint64_t*, dgr_taken*);
typedef uint64_t (*takes_words_fn)(int, const uint64_t*);
typedef uint64_t (*takes_pack_fn)(uint64_t*, uint64_t*, int, const uint64_t* const*, const uint64_t*,
                                  const uint64_t**, uint64_t*);
take_keysets_fn f = dg_take_keysets;
take_batch_fn g = dgr_take_batch;
takes_words_fn w = dgr_takes_words;
takes_pack_fn p = dgr_takes_pack;
_Static_assert(DG_ABI_VERSION == 4, "the addition is additive");
"""

# dgr_taken's size and member offsets, as the C compiler has them
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "replica.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dgr_taken), offsetof(dgr_taken, n_keys), offsetof(dgr_taken, keys),
         offsetof(dgr_taken, masks), offsetof(dgr_taken, offs), offsetof(dgr_taken, rows));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


@pytest.fixture(scope="module")
def rlib(lib):
    if not os.path.exists(nif.LIB_PATH):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    return nif.load()


def test_prototypes_compile_and_the_struct_layout_matches(tmp_path, lib):
    src, exe = tmp_path / "proto.c", tmp_path / "proto"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(src), "-o", str(tmp_path / "proto.o")], check=True)
    bad = tmp_path / "bad.c"
    bad.write_text(PROTO_C.replace("uint64_t, uint64_t*, dg_store*);", "uint64_t, uint64_t*);"))
    assert subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(bad), "-o", str(tmp_path / "bad.o")],
                          capture_output=True).returncode != 0
    layout = tmp_path / "layout.c"
    layout.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, str(layout), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = nif.dgr_taken
    assert got == [C.sizeof(T), T.n_keys.offset, T.keys.offset, T.masks.offset, T.offs.offset, T.rows.offset]
    assert T.rows.size == C.sizeof(_abi.dg_store)
    assert lib.dg_abi_version() == 4
    S = C.POINTER(_abi.dg_store)
    assert _abi._SIGS["dg_take_keysets"] == (C.c_int, [C.c_void_p, S, C.c_int, C.POINTER(C.c_void_p), _abi.P64,
                                                       _abi.P64, _abi.P64, _abi.P64, C.c_uint64, _abi.P64, S])
    assert len(_abi._SIGS["dg_take_keysets"][1]) == 11  # the arguments of take_keysets_fn above
    assert lib.dg_take_keysets.argtypes == _abi._SIGS["dg_take_keysets"][1]
    assert len(nif._SIGS["dgr_take_batch"][1]) == 6 and len(nif._SIGS["dgr_takes_pack"][1]) == 7


def test_entry_points_are_exported_and_reject_bad_arguments(lib, rlib):
    """Validation comes before any device call, so it is the same without a GPU."""
    assert "dg_take_keysets" in set(_abi.header_functions())
    for name in ("dgr_take_batch", "dgr_takes_words", "dgr_takes_pack"):
        assert getattr(rlib, name) is not None
    s, out = _abi.dg_store(), _abi.dg_store()
    n = C.c_uint64(7)
    offs = (C.c_uint64 * 4)()
    call = lambda e, k, keys, nk, uk, mk, of, cap, nu, o: lib.dg_take_keysets(e, C.byref(s), k, keys, nk, uk, mk, of,
                                                                               cap, nu, o)
    assert call(None, 0, None, None, None, None, offs, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    # with an engine-shaped pointer the argument checks run before the engine is used
    fake = C.c_void_p(1)
    assert call(fake, 0, None, None, None, None, offs, 0, None, C.byref(out)) == _abi.DG_E_INVAL
    assert call(fake, 0, None, None, None, None, offs, 0, C.byref(n), None) == _abi.DG_E_INVAL
    assert call(fake, 0, None, None, None, None, None, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert n.value == 0  # (written before the checks that can fail)
    kp = (C.c_void_p * 65)()
    nk = (C.c_uint64 * 65)()
    assert call(fake, 65, kp, nk, None, None, offs, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert b"65 keysets" in lib.dg_last_error()
    assert call(fake, -1, kp, nk, None, None, offs, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert call(fake, 1, None, nk, None, None, offs, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert call(fake, 1, kp, None, None, None, offs, 0, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    nk[0] = 3  # a null keyset with keys in it; output arrays missing for cap_keys > 0
    assert call(fake, 1, kp, nk, offs, offs, offs, 3, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert b"keys NULL with n_keys>0" in lib.dg_last_error()
    assert call(fake, 0, None, None, None, None, offs, 3, C.byref(n), C.byref(out)) == _abi.DG_E_INVAL
    assert b"null output array" in lib.dg_last_error()
    # the replica layer: null state or result, k out of range, keysets missing
    tk = nif.dgr_taken()
    assert rlib.dgr_take_batch(None, 0, 0, None, None, C.byref(tk)) == _abi.DG_E_INVAL
    assert rlib.dgr_take_batch(fake, 0, 0, None, None, None) == _abi.DG_E_INVAL
    assert rlib.dgr_take_batch(fake, 0, 65, kp, nk, C.byref(tk)) == _abi.DG_E_INVAL
    assert rlib.dgr_take_batch(fake, 0, -1, kp, nk, C.byref(tk)) == _abi.DG_E_INVAL
    assert rlib.dgr_take_batch(fake, 0, 1, None, nk, C.byref(tk)) == _abi.DG_E_INVAL
    assert rlib.dgr_take_batch(fake, 0, 1, kp, nk, C.byref(tk)) == _abi.DG_E_INVAL  # keys[0] NULL, n_keys[0] = 3
    assert rlib.dgr_takes_words(0, None) == 0
    sizes = (C.c_uint64 * 3)(3, 0, 4)
    assert rlib.dgr_takes_words(3, sizes) == 8  # 3 keys take 4 words
