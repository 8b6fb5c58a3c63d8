"""The stream join's stripe-count recurrence (csrc/dg_jstripe.h) on the host:
tests/stripe_prefix.cc, built with ASan and UBSan, walks every workgroup of grids of 1 to
1,024 through joins that end in every kind of last stripe and compares each tile's offset
and the total with a plain prefix sum over the tiles' counts; no lane may load a granule
outside the tiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_crdt_ex_amd", "csrc")


def test_stripe_prefix(tmp_path):
    exe = str(tmp_path / "stripe_prefix")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "stripe_prefix.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
