"""sdiff_layout (csrc/dg_arena.h), the streaming store diff's scratch, on the host:
tests/arena_layout_sdiff.cc, a stand-alone program built with ASan and UBSan, checks its
regions (inside the buffer, 256-byte padded, disjoint, writable end to end) and that the mask
covers every word the kernels touch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_sdiff_layout(tmp_path):
    exe = str(tmp_path / "arena_layout_sdiff")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layout_sdiff.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_restated_constants_are_the_launchers():
    """The tile and the mask size the .cc restates are csrc/dg_launch.h's."""
    text = open(os.path.join(CSRC, "dg_launch.h")).read()
    assert "constexpr u64 SDIFF_TILE = 2048;" in text
    assert "return (na + nb) / 32 + SDIFF_TILE / 32 + 4;" in text
