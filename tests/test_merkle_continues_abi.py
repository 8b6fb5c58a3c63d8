"""dg_merkle_continues and dgr_merkle_continue_batch at their boundaries without a GPU: the
prototypes compile from the headers with gcc and take the arguments the ctypes tables declare,
dg_cont_hop and dgr_cont_result are laid out in _abi.py / nif.py as the C compiler lays them
out, the libraries export the entry points, the ABI version is still 4, and bad arguments are
rejected before any device call.  The output carve of the replica layer (replica_pack.h
rp_cont_carve) is checked by c_src/test_carve.c, a stand-alone program built here with ASan
and UBSan."""
import ctypes as C
import os
import subprocess

import pytest

from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "c_src")]

PROTO_C = r"""
#include "replica.h"
typedef int (*continues_fn)(dg_engine*, const dg_merkle*, const dg_store*, int, dg_cont_hop*, uint32_t, uint64_t);
typedef int (*continue_batch_fn)(dgr_state*, uint64_t, int, const uint8_t* const*, const uint64_t*, uint32_t,
                                 uint64_t, dgr_cont_result*);
continues_fn f = dg_merkle_continues;
continue_batch_fn g = dgr_merkle_continue_batch;
_Static_assert(DG_ABI_VERSION == 4, "the addition is additive");
_Static_assert(DG_CONT_BATCH_MAX == 64, "a batch is at most 64 hops");
"""

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "replica.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dg_cont_hop), offsetof(dg_cont_hop, in),
         offsetof(dg_cont_hop, out), offsetof(dg_cont_hop, keys), offsetof(dg_cont_hop, cap),
         offsetof(dg_cont_hop, n_keys), offsetof(dg_cont_hop, n_total), offsetof(dg_cont_hop, status),
         offsetof(dg_cont_hop, rc));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(dgr_cont_result), offsetof(dgr_cont_result, rc),
         offsetof(dgr_cont_result, status), offsetof(dgr_cont_result, bin), offsetof(dgr_cont_result, len),
         offsetof(dgr_cont_result, keys), offsetof(dgr_cont_result, n_keys));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


@pytest.fixture(scope="module")
def rlib(lib):
    if not os.path.exists(nif.LIB_PATH) or not hasattr(C.CDLL(nif.LIB_PATH), "dgr_merkle_continue_batch"):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    return nif.load()


def test_prototypes_compile_and_the_struct_layouts_match(tmp_path, lib):
    src, exe = tmp_path / "proto.c", tmp_path / "layout"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(src), "-o", str(tmp_path / "proto.o")], check=True)
    bad = tmp_path / "bad.c"
    bad.write_text(PROTO_C.replace("dg_cont_hop*, uint32_t, uint64_t);", "dg_cont_hop*, uint32_t);"))
    assert subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(bad), "-o", str(tmp_path / "bad.o")],
                          capture_output=True).returncode != 0
    layout = tmp_path / "layout.c"
    layout.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, str(layout), "-o", str(exe)], check=True)
    hop, res = (
        [int(x) for x in line.split()]
        for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    H = _abi.dg_cont_hop
    assert hop == [C.sizeof(H), H.in_.offset, H.out.offset, H.keys.offset, H.cap.offset, H.n_keys.offset,
                   H.n_total.offset, H.status.offset, H.rc.offset]
    T = nif.dgr_cont_result
    assert res == [C.sizeof(T), T.rc.offset, T.status.offset, T.bin.offset, T.len.offset, T.keys.offset,
                   T.n_keys.offset]
    assert lib.dg_abi_version() == 4
    assert _abi.DG_CONT_BATCH_MAX == 64 == nif.CONT_BATCH_MAX
    sig = _abi._SIGS["dg_merkle_continues"]
    assert sig == (C.c_int, [C.c_void_p, C.POINTER(_abi.dg_merkle), C.POINTER(_abi.dg_store), C.c_int,
                             C.POINTER(H), C.c_uint32, C.c_uint64])
    assert lib.dg_merkle_continues.argtypes == sig[1]
    assert len(nif._SIGS["dgr_merkle_continue_batch"][1]) == 8  # the arguments of continue_batch_fn above


def _tree():
    """a tree that passes the shape checks (its arrays are never read before a launch)"""
    t = _abi.dg_merkle()
    t.depth = 8
    t.nodes = 64
    t.counts = 64
    return t


def test_the_call_rejects_bad_arguments_before_any_launch(lib):
    """Validation comes before any device call, so it is the same without a GPU."""
    assert "dg_merkle_continues" in set(_abi.header_functions())
    t, s = _tree(), _abi.dg_store()
    hops = (_abi.dg_cont_hop * 65)()
    call = lambda e, tt, ss, k, h, levels: lib.dg_merkle_continues(e, tt, ss, k, h, levels, 5)
    assert call(None, C.byref(t), C.byref(s), 0, hops, 3) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    fake = C.c_void_p(1)  # engine-shaped: the argument checks run before the engine is used
    assert call(fake, None, C.byref(s), 1, hops, 3) == _abi.DG_E_INVAL
    assert call(fake, C.byref(_abi.dg_merkle()), C.byref(s), 1, hops, 3) == _abi.DG_E_INVAL
    assert call(fake, C.byref(t), None, 1, hops, 3) == _abi.DG_E_INVAL
    assert call(fake, C.byref(t), C.byref(s), 65, hops, 3) == _abi.DG_E_INVAL
    assert b"65 hops" in lib.dg_last_error()
    assert call(fake, C.byref(t), C.byref(s), -1, hops, 3) == _abi.DG_E_INVAL
    assert call(fake, C.byref(t), C.byref(s), 1, None, 3) == _abi.DG_E_INVAL
    assert call(fake, C.byref(t), C.byref(s), 1, hops, 0) == _abi.DG_E_INVAL
    assert call(fake, C.byref(t), C.byref(s), 0, None, 3) == _abi.DG_OK  # no hop: no launch, no wait


def test_hops_that_need_no_workgroup_are_answered_on_the_host(lib):
    """A declined hop, an empty input, a null input and a level past the leaves in one batch:
    each gets its own status and rc, the call returns DG_OK and the engine is never used."""
    t, s = _tree(), _abi.dg_store()
    words = (C.c_uint64 * 8)()
    p = C.cast(words, C.c_void_p)
    big = _abi.dg_merkle_cont(level=3, pos=p, hash=p, n=4097)                         # over the entries
    wide = _abi.dg_merkle_cont(level=9, pos=p, hash=p, n=4, bucket=p, n_buckets=513)  # over the buckets
    empty = _abi.dg_merkle_cont(level=3, n=0)
    empty_leaf = _abi.dg_merkle_cont(level=9, pos=p, hash=p, n=4)
    null_in = _abi.dg_merkle_cont(level=3, n=4)
    deep = _abi.dg_merkle_cont(level=10, pos=p, hash=p, n=4)
    ins = [big, wide, empty, empty_leaf, null_in, deep, None]
    hops = (_abi.dg_cont_hop * len(ins))()
    for h, c in zip(hops, ins):
        if c is not None:
            h.in_ = C.pointer(c)
        h.n_keys = h.n_total = 77  # (reset by the call)
        h.status = h.rc = 77
    assert lib.dg_merkle_continues(C.c_void_p(1), C.byref(t), C.byref(s), len(ins), hops, 3, 5) == _abi.DG_OK
    assert [(h.status, h.rc) for h in hops] == [
        (_abi.DG_CONT_DECLINED, 0), (_abi.DG_CONT_DECLINED, 0), (0, 0), (0, 0),
        (0, _abi.DG_E_INVAL), (0, _abi.DG_E_INVAL), (0, _abi.DG_E_INVAL)]
    assert all(h.n_keys == 0 and h.n_total == 0 for h in hops)
    assert b"hop 4: null input" in lib.dg_last_error()  # the first hop whose rc is not DG_OK


def test_the_replica_call_rejects_bad_arguments(rlib):
    fake = C.c_void_p(1)
    bins = (C.c_char_p * 65)()
    lens = (C.c_uint64 * 65)()
    res = (nif.dgr_cont_result * 65)()
    f = rlib.dgr_merkle_continue_batch
    assert f(None, 0, 0, bins, lens, 3, 5, res) == _abi.DG_E_INVAL
    assert f(fake, 0, -1, bins, lens, 3, 5, res) == _abi.DG_E_INVAL
    assert f(fake, 0, 65, bins, lens, 3, 5, res) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, None, lens, 3, 5, res) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, None, 3, 5, res) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, lens, 3, 5, None) == _abi.DG_E_INVAL


def test_output_carve_under_sanitizers(tmp_path):
    """c_src/test_carve.c: the hops' regions of the one staging block are disjoint, 8-byte
    aligned and sized by the single hop's formulas, k = 1 .. 64 at the limits."""
    exe = str(tmp_path / "test_carve")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", *INC,
                    os.path.join(ROOT, "c_src", "test_carve.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "157 cases" in r.stdout, r.stdout[-2000:]
