"""The packed message of a batch of keysets (c_src/replica_pack.c dgr_takes_words / dgr_takes_pack)
on the host: c_src/test_takes.c, a plain executable, checks that every keyset lies sorted and
unique at its documented 16-byte aligned offset (given unsorted with duplicates, ascending
already, or ascending but for one pair), that the device views name the same places,
that no keyset leaves the message, k = 0 and empty keysets, and the word count against the
sizing function's.  No device is opened."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "c_src", "_build", "test_takes")


def test_takes_packing():
    # built by __graft_entry__.build(); rebuilt here only when absent
    if not os.path.exists(EXE):
        from oracle import ref
        ref.build()
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src")], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "1006 cases" in r.stdout, r.stdout[-2000:]
