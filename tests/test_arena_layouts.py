"""The C-ABI layer's scratch layouts (csrc/dg_arena.h) on the host: tests/arena_layouts.cc,
built with ASan and UBSan, checks every layout's regions (inside the buffer, aligned, not
overlapping, writable at both ends) and their offsets against the formulas the layer used
while it was one file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_arena_layouts(tmp_path):
    exe = str(tmp_path / "arena_layouts")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layouts.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
