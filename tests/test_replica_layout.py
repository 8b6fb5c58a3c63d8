"""The replica layer's host layouts (c_src/replica_pack.h) on the host: c_src/test_layout.c, a
plain executable, checks the return block's regions for a grid of (S, C) -- aligned, disjoint,
inside the size function's figure, at the word offsets the kernels and the term layers know --
the rows and context view constructors' column order, the S that gives n bytes at the block's
head, and the continuation frame's write / parse round trip and rejections.  No device is
opened."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "c_src", "_build", "test_layout")


def test_replica_layouts():
    # built by __graft_entry__.build(); rebuilt here only when absent
    if not os.path.exists(EXE):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "50 cases" in r.stdout, r.stdout[-2000:]
