"""The packed message of a batch of deltas (c_src/replica_pack.c dgr_batch_words / dgr_batch_pack)
on the host: c_src/test_batch.c, a plain executable, checks the offsets of every delta's rows,
context and keyset, their 16-byte alignment, that they neither overlap nor leave the message,
their contents, and the keysets' sort-unique.  No device is opened."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "c_src", "_build", "test_batch")


def test_batch_packing():
    # built by __graft_entry__.build(); rebuilt here only when absent
    if not os.path.exists(EXE):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "1002 cases" in r.stdout, r.stdout[-2000:]
