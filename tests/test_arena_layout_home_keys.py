"""home_layout (csrc/dg_arena.h) with dg_mutate_home's touched-keys array, on the host:
tests/arena_layout_home_keys.cc, a stand-alone program built with ASan and UBSan, checks that
the array stands where the layout's unused sixth per-key array stood, that no offset behind it
moved, and that every region is inside the buffer, 256-byte padded, disjoint and writable."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_home_layout_with_the_touched_keys(tmp_path):
    exe = str(tmp_path / "arena_layout_home_keys")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layout_home_keys.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_restated_constants_are_the_launchers():
    text = open(os.path.join(CSRC, "dg_launch.h")).read()
    assert "SMALL_TAKEN = 1024, SMALL_EDIT = 1536;" in text
    assert "constexpr u64 SMALL_WORDS = SMALL_O_CTX + SMALL_NODES + SMALL_NODES / 2;" in text
