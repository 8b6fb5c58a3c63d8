"""keyed_layout (csrc/dg_arena.h), dg_join_deltas_keyed's scratch, on the host:
tests/arena_layout_keyed.cc, a stand-alone program built with ASan and UBSan, checks its
regions (inside the buffer, 256-byte padded, disjoint, writable end to end, the words zeroed
per call, the one-wait path's arrays sized for every item)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_keyed_layout(tmp_path):
    exe = str(tmp_path / "arena_layout_keyed")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layout_keyed.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_restated_constants_are_the_launchers():
    """What the .cc restates is csrc/dg_launch.h's: KsSeg (16 bytes), KRun (96 bytes: Rows of
    five pointers and n, keys, n_keys, Ctx of two pointers, n and kind), KNT, KD_BLOCK, KD_NV."""
    text = open(os.path.join(CSRC, "dg_launch.h")).read()
    assert "struct KsSeg {" in text and "  const u64* keys;\n  u64 off;" in text
    assert re.search(r"struct KRun \{[^}]*\n  Rows rows;\n  const u64\* keys;\n  u64 n_keys;\n  Ctx ctx;\n\};", text)
    assert "constexpr int KNT = 1024;" in text and "constexpr int KD_BLOCK = 256;" in text
    assert "constexpr int KD_NV = 7;" in text
