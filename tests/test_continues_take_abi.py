"""dg_merkle_continues_take and dgr_merkle_continue_take_batch at their boundaries without a GPU:
the prototypes compile from the headers with gcc and take the arguments the ctypes tables declare,
dg_cont_take and dgr_hop_rows are laid out in _abi.py / nif.py as the C compiler lays them out, the
libraries export the entry points, the ABI version is still 4, the calls' own DG_E_INVAL cases are
rejected before any device call, and a batch of hops that need no workgroup is answered on the host
with no rows.  The row rooms of the replica layer (replica_pack.h rp_take_carve) are checked by
c_src/test_carve_take.c, a stand-alone program built here with ASan and UBSan."""
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
typedef int (*take_batch_fn)(dgr_state*, uint64_t, int, const uint8_t* const*, const uint64_t*, const uint8_t*,
                             uint32_t, uint64_t, dgr_cont_result*, dgr_hop_rows*);
take_batch_fn g = dgr_merkle_continue_take_batch;
typedef int (*take_fn)(dg_engine*, const dg_merkle*, const dg_store*, int, dg_cont_hop*, dg_cont_take* const*,
                       uint32_t, uint64_t);
take_fn f = dg_merkle_continues_take;
_Static_assert(DG_ABI_VERSION == 4, "the addition is additive");
"""

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "replica.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(dgr_hop_rows), offsetof(dgr_hop_rows, rows), offsetof(dgr_hop_rows, offs));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dg_cont_take), offsetof(dg_cont_take, rows), offsetof(dg_cont_take, offs),
         offsetof(dg_cont_take, rc), offsetof(dg_cont_take, rows.n), offsetof(dg_cont_take, rows.cap));
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_prototype_compiles_and_the_struct_layout_matches(tmp_path, lib):
    src = tmp_path / "proto.c"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(src), "-o", str(tmp_path / "proto.o")], check=True)
    bad = tmp_path / "bad.c"
    bad.write_text(PROTO_C.replace("dg_cont_take* const*,", ""))
    assert subprocess.run(["gcc", "-Wall", "-Werror", *INC, "-c", str(bad), "-o", str(tmp_path / "bad.o")],
                          capture_output=True).returncode != 0
    layout, exe = tmp_path / "layout.c", tmp_path / "layout"
    layout.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-Wall", "-Werror", *INC, str(layout), "-o", str(exe)], check=True)
    hr, got = ([int(x) for x in line.split()]
               for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    H = nif.dgr_hop_rows
    assert hr == [C.sizeof(H), H.rows.offset, H.offs.offset]
    assert len(nif._SIGS["dgr_merkle_continue_take_batch"][1]) == 10  # the arguments of take_batch_fn above
    T, S = _abi.dg_cont_take, _abi.dg_store
    assert got == [C.sizeof(T), T.rows.offset, T.offs.offset, T.rc.offset, T.rows.offset + S.n.offset,
                   T.rows.offset + S.cap.offset]
    assert lib.dg_abi_version() == 4
    assert "dg_merkle_continues_take" in set(_abi.header_functions())
    sig = _abi._SIGS["dg_merkle_continues_take"]
    assert sig == (C.c_int, [C.c_void_p, C.POINTER(_abi.dg_merkle), C.POINTER(_abi.dg_store), C.c_int,
                             C.POINTER(_abi.dg_cont_hop), C.POINTER(C.POINTER(T)), C.c_uint32, C.c_uint64])
    assert lib.dg_merkle_continues_take.argtypes == sig[1]


def _tree():
    """a tree that passes the shape checks (its arrays are never read before a launch)"""
    t = _abi.dg_merkle()
    t.depth = 8
    t.nodes = 64
    t.counts = 64
    return t


def _takes(*ts):
    arr = (C.POINTER(_abi.dg_cont_take) * max(len(ts), 1))()
    for i, t in enumerate(ts):
        if t is not None:
            arr[i] = C.pointer(t)
    return arr


def test_the_call_rejects_bad_arguments_before_any_launch(lib):
    """dg_merkle_continues' call-level cases and the take's own, with an engine that is never used."""
    t, s = _tree(), _abi.dg_store()
    fake = C.c_void_p(1)
    words = (C.c_uint64 * 16)()
    p = C.cast(words, C.c_void_p)
    cont = _abi.dg_merkle_cont(level=9, pos=p, hash=p, n=4, bucket=p, n_buckets=1)
    hops = (_abi.dg_cont_hop * 65)()
    hops[0].in_ = C.pointer(cont)
    hops[0].keys = p
    hops[0].cap = 4
    good = _abi.dg_cont_take(rows=_abi.dg_store(p, p, p, p, p, 0, 2), offs=p)
    call = lambda e, k, h, tk, levels=3: lib.dg_merkle_continues_take(e, C.byref(t), C.byref(s), k, h, tk, levels, 5)
    assert call(None, 1, hops, _takes(good)) == _abi.DG_E_INVAL
    assert b"null engine" in lib.dg_last_error()
    assert call(fake, 65, hops, _takes(*[None] * 65)) == _abi.DG_E_INVAL
    assert b"dg_merkle_continues_take: k = 65 hops" in lib.dg_last_error()
    assert call(fake, -1, hops, _takes(good)) == _abi.DG_E_INVAL
    assert call(fake, 1, None, _takes(good)) == _abi.DG_E_INVAL
    assert call(fake, 1, hops, _takes(good), 0) == _abi.DG_E_INVAL
    assert call(fake, 0, None, None) == _abi.DG_OK  # no hop: no launch, no wait
    # the take's own cases
    assert call(fake, 1, hops, _takes(_abi.dg_cont_take(rows=good.rows))) == _abi.DG_E_INVAL
    assert b"take 0: null offs" in lib.dg_last_error()
    for col in ("key", "val", "ts", "node", "cnt"):
        rows = _abi.dg_store(p, p, p, p, p, 0, 2)
        setattr(rows, col, None)
        assert call(fake, 1, hops, _takes(_abi.dg_cont_take(rows=rows, offs=p))) == _abi.DG_E_INVAL
        assert b"take 0: null column with cap=2" in lib.dg_last_error()
    hops[1].in_ = C.pointer(cont)  # a hop with a take but no room for keys
    hops[1].keys, hops[1].cap = None, 4
    assert call(fake, 2, hops, _takes(None, good)) == _abi.DG_E_INVAL
    assert b"take 1: its hop has no room for keys" in lib.dg_last_error()
    hops[1].keys, hops[1].cap = p, 0
    assert call(fake, 2, hops, _takes(None, good)) == _abi.DG_E_INVAL


def test_hops_that_need_no_workgroup_are_answered_on_the_host_without_rows(lib):
    """A declined hop, an empty node form, an empty leaf form and a null input, each with a take:
    statuses and rcs as dg_merkle_continues gives them, rows.n = 0 and rc = DG_OK in every take,
    and the engine is never used."""
    t, s = _tree(), _abi.dg_store()
    words = (C.c_uint64 * 8)()
    p = C.cast(words, C.c_void_p)
    ins = [_abi.dg_merkle_cont(level=9, pos=p, hash=p, n=4, bucket=p, n_buckets=513),  # over the buckets
           _abi.dg_merkle_cont(level=3, n=0),
           _abi.dg_merkle_cont(level=9, pos=p, hash=p, n=4),                           # no buckets: {:ok, []}
           _abi.dg_merkle_cont(level=3, n=4)]                                          # null input
    hops = (_abi.dg_cont_hop * len(ins))()
    takes = [_abi.dg_cont_take(rows=_abi.dg_store(p, p, p, p, p, 77, 1), offs=p, rc=77) for _ in ins]
    for h, c in zip(hops, ins):
        h.in_ = C.pointer(c)
        h.keys, h.cap = p, 1
        h.status = h.rc = 77
    assert lib.dg_merkle_continues_take(C.c_void_p(1), C.byref(t), C.byref(s), len(ins), hops, _takes(*takes),
                                        3, 5) == _abi.DG_OK
    assert [(h.status, h.rc) for h in hops] == [(_abi.DG_CONT_DECLINED, 0), (0, 0), (0, 0), (0, _abi.DG_E_INVAL)]
    assert all(tk.rows.n == 0 and tk.rc == _abi.DG_OK for tk in takes)
    assert b"dg_merkle_continues_take: hop 3: null input" in lib.dg_last_error()
    # takes == NULL: the call is dg_merkle_continues
    assert lib.dg_merkle_continues_take(C.c_void_p(1), C.byref(t), C.byref(s), len(ins), hops, None, 3, 5) == _abi.DG_OK
    assert b"dg_merkle_continues: hop 3: null input" in lib.dg_last_error()


@pytest.fixture(scope="module")
def rlib(lib):
    if not os.path.exists(nif.LIB_PATH) or not hasattr(C.CDLL(nif.LIB_PATH), "dgr_merkle_continue_take_batch"):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    return nif.load()


def test_the_replica_call_rejects_bad_arguments(rlib):
    fake = C.c_void_p(1)
    bins = (C.c_char_p * 65)()
    lens = (C.c_uint64 * 65)()
    res = (nif.dgr_cont_result * 65)()
    taken = (nif.dgr_hop_rows * 65)()
    want = bytes(65)
    f = rlib.dgr_merkle_continue_take_batch
    assert f(None, 0, 0, bins, lens, want, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, -1, bins, lens, want, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 65, bins, lens, want, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, None, lens, want, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, None, want, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, lens, None, 3, 5, res, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, lens, want, 3, 5, None, taken) == _abi.DG_E_INVAL
    assert f(fake, 0, 1, bins, lens, want, 3, 5, res, None) == _abi.DG_E_INVAL


def test_row_room_carve_under_sanitizers(tmp_path):
    """c_src/test_carve_take.c: the hops' row columns and offsets are disjoint, 8-byte aligned and
    sized by the formulas beside the untouched output carve, k = 1 .. 64 at the limits."""
    exe = str(tmp_path / "test_carve_take")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", *INC,
                    os.path.join(ROOT, "c_src", "test_carve_take.c"), os.path.join(ROOT, "c_src", "replica_pack.c"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "792 cases" in r.stdout, r.stdout[-2000:]
