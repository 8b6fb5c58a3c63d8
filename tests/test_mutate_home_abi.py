"""dg_mutate_home[_diffs] and the replica layer's additions at their C boundaries, without a
GPU: the header declares and the library exports both entry points, their prototypes compile
against deltagpu.h as the issue states them, the ctypes mirror agrees, the ABI version is still
4, replica.h's dgr_mutate_route_stats / dgr_mutate_pack match nif.py, and null arguments are
refused before any device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from delta_crdt_ex_amd import _abi, nif
from delta_crdt_ex_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTO_C = r"""
#include <stdio.h>
#include "replica.h"
/* a prototype that differs from the header's is a compile error */
int dg_mutate_home(dg_engine*, dg_store* state, dg_context* state_ctx, uint32_t node, uint64_t m,
                   const uint8_t* kind, const uint64_t* key, const uint64_t* val, const int64_t* ts,
                   const uint64_t* add_rank, uint64_t n_adds, dg_store* spare, dg_merkle* tree,
                   uint64_t* home, int* swapped);
int dg_mutate_home_diffs(dg_engine*, dg_store* state, dg_context* state_ctx, uint32_t node, uint64_t m,
                         const uint8_t* kind, const uint64_t* key, const uint64_t* val, const int64_t* ts,
                         const uint64_t* add_rank, uint64_t n_adds, dg_store* spare, dg_merkle* tree,
                         uint64_t* home, int* swapped);
int dgr_mutate_route_stats(const dgr_engine* g, uint64_t out[3]);
uint64_t dgr_mutate_words(uint64_t m);
int dgr_mutate_pack(uint64_t* host, uint64_t m, const uint8_t* kind, const uint64_t* key, const uint64_t* val,
                    const int64_t* ts, uint64_t* n_adds);
int main(void) {
  printf("%d %d %d %d\n", DG_ABI_VERSION, DGR_MUTATE_TRIED, DGR_MUTATE_SERVED, DGR_MUTATE_DECLINED);
  return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    build()
    return _abi.load()


def test_prototypes_compile_against_the_headers(tmp_path):
    src, exe = tmp_path / "proto.c", tmp_path / "proto"
    src.write_text(PROTO_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "c_src"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [4, 0, 1, 2]


def test_header_library_and_mirror_have_the_entry_points(lib):
    for name in ("dg_mutate_home", "dg_mutate_home_diffs"):
        assert name in _abi.header_functions()
        assert hasattr(lib, name)
    # one signature: dg_mutate_batch's op arguments between dg_join_delta_home's state and outputs
    sig = _abi._SIGS["dg_mutate_home"]
    assert _abi._SIGS["dg_mutate_home_diffs"] == sig
    home, batch = _abi._SIGS["dg_join_delta_home"][1], _abi._SIGS["dg_mutate_batch"][1]
    assert sig[0] is C.c_int and sig[1] == home[:3] + batch[3:11] + home[7:]
    assert lib.dg_abi_version() == 4


def test_replica_header_declares_the_route_stats_and_the_packer():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "c_src", "replica.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dgr_mutate_route_stats\s*\(\s*const\s+dgr_engine\s*\*\s*g\s*,\s*uint64_t\s+out\[3\]\s*\)", text)
    assert re.search(r"\bint\s+dgr_mutate_pack\s*\(", text) and re.search(r"\buint64_t\s+dgr_mutate_words\s*\(", text)
    assert nif._SIGS["dgr_mutate_route_stats"] == nif._SIGS["dgr_deltas_route_stats"]
    # deltagpu_nif.c reaches the new call through dgr_mutate_batch[_diffs] alone
    nif_c = open(os.path.join(ROOT, "c_src", "deltagpu_nif.c")).read()
    assert "dg_mutate_home" not in nif_c and "dgr_mutate_batch" in nif_c


def test_null_arguments_are_refused_before_any_device_call(lib):
    st, cx = _abi.dg_store(), _abi.dg_context()
    sw = C.c_int(0)
    home = (C.c_uint64 * _abi.DG_HOME_DIFFS_WORDS)()
    for f in (lib.dg_mutate_home, lib.dg_mutate_home_diffs):
        assert f(None, C.byref(st), C.byref(cx), 1, 0, None, None, None, None, None, 0, C.byref(st), None, home,
                 C.byref(sw)) == _abi.DG_E_INVAL
