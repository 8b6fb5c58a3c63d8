"""takesets_layout (csrc/dg_arena.h), dg_take_keysets' scratch, on the host:
tests/arena_layout_takesets.cc, a stand-alone program built with ASan and UBSan, checks its
regions (inside the buffer, 256-byte padded, disjoint, writable end to end, the per-key offsets
through their extra entry)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_takesets_layout(tmp_path):
    exe = str(tmp_path / "arena_layout_takesets")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layout_takesets.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_restated_descriptor_is_the_launchers():
    """The descriptor the .cc sizes (16 bytes) is csrc/dg_launch.h's KsSeg: a pointer and a u64."""
    text = open(os.path.join(CSRC, "dg_launch.h")).read()
    assert "struct KsSeg {" in text and "  const u64* keys;\n  u64 off;" in text
