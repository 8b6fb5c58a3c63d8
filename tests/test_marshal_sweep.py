"""The C universe's sweeps (c_src/marshal.c dgm_sweep_values / dgm_sweep_keys) through the
stand-alone program c_src/_build/test_sweep (host only: no device, so it may be started from
a test).  The program checks itself -- a flag array of the wrong length gives DG_E_INVAL,
keeps minus drops equals the live entries, every key lookup works after the map's rebuild --
and prints the ids of "intern 3000 values, sweep two thirds, intern 500 more", which must be
the Python Universe's for the same sequence."""
import os
import subprocess

import numpy as np
import pytest

from delta_crdt_ex_amd.interning import Universe
from delta_crdt_ex_amd.terms import order_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "c_src", "_build", "test_sweep")
N1, N2 = 3000, 500


@pytest.fixture(scope="module")
def program_output():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src"), "_build/test_sweep"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_program_checks_pass(program_output):
    """n mismatch -> DG_E_INVAL, keeps - drops == live entries, key lookups after the rebuild:
    the program's own CHECKs (c_src/test_sweep.c), exit status 0."""
    rc, out, err = program_output
    assert rc == 0, err
    assert out.rstrip().endswith("test_sweep: ok")


def seq_value(i):
    """value i of test_sweep.c's sequence"""
    x = (i * 2654435761) & 0xFFFFFFFF
    return x / 7.0 if i % 3 == 0 else "s%08x" % x


def test_ids_equal_the_python_universes(program_output):
    rc, out, _err = program_output
    assert rc == 0
    got = {int(a): int(b) for _tag, a, b in (ln.split() for ln in out.splitlines() if ln.startswith("ID "))}
    U = Universe()
    for i in range(N1):
        U.value(seq_value(i))
    ids, terms = U.value_ids()
    live = {order_key(seq_value(i)) for i in range(N1) if i % 3 == 1}
    dropped = U.sweep(np.array([order_key(t) in live for t in terms], np.uint8))
    assert dropped["values"] == (N1, N1 // 3)
    for i in range(N2):
        U.value(seq_value(N1 + i if i % 2 else 3 * i))
    ids, terms = U.value_ids()
    by_term = dict(zip(map(order_key, terms), ids))
    want = {i: by_term[order_key(seq_value(i))] for i in range(N1 + N2) if order_key(seq_value(i)) in by_term}
    assert len(want) == N1 // 3 + N2
    assert got == want
