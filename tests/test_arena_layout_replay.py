"""replay_layout (csrc/dg_arena.h), dg_replace_keysets' scratch, on the host:
tests/arena_layout_replay.cc, a stand-alone program built with ASan and UBSan, checks its
regions (inside the buffer, 256-byte padded, disjoint, writable end to end, the edit offsets
through their extra entry)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_replay_layout(tmp_path):
    exe = str(tmp_path / "arena_layout_replay")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "arena_layout_replay.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_restated_tile_is_the_launchers():
    """The union tile the .cc sizes the tile arrays by (1024 items) is csrc/dg_launch.h's."""
    text = open(os.path.join(CSRC, "dg_launch.h")).read()
    assert "constexpr int RP_BLOCK = 256;" in text and "constexpr int RP_ITEMS = 4;" in text
    assert "constexpr int RP_TILE = RP_BLOCK * RP_ITEMS;" in text
