"""dgr_mutate_pack (c_src/replica_pack.c), the packed message of dgr_mutate_batch's ops, on the
host: c_src/test_mutate_pack.c -- keys out of order in the batch, equal keys keeping batch
order, ranks, m = 0 / 1 / 512 / 513 -- built plainly and under ASan + UBSan (a plain executable,
nothing preloaded), and run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SRC = os.path.join(ROOT, "c_src")


@pytest.mark.parametrize("target", ["test_mutate_pack", "test_mutate_pack_asan"])
def test_mutate_pack(target):
    subprocess.run(["make", "-s", "-C", C_SRC, "_build/" + target], check=True)
    r = subprocess.run([os.path.join(C_SRC, "_build", target)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and not r.stdout.startswith("0 cases")
