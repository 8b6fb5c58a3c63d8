"""on_diffs' term-layer half without a GPU: c_src/test_diffs.c (dgm_value_find and
dgm_classify_diffs over the full table of flags, equal / different values, nil on either side
and nil never interned) passes, the Python helper behind nif.py classifies every row of that
table as the C function does, and interning.Universe.value_find looks a value up without
interning it."""
import os
import subprocess

import pytest

from delta_crdt_ex_amd import interning, nif
from delta_crdt_ex_amd.terms import Atom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "c_src", "_build", "test_diffs")


@pytest.fixture(scope="module")
def rows():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "c_src"), "_build/test_diffs"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [[int(x) for x in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("ROW ")]
    assert "test_diffs ok" in r.stdout
    return out


def test_c_table_is_complete(rows):
    """28 rows: (5 value shapes with nil interned + 2 without) x 4 flag pairs; every kind occurs."""
    assert len(rows) == 28
    assert {(of, nf) for of, nf, *_ in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r[4] for r in rows} == {0, 1} and {r[6] for r in rows} == {0, 1, 2}


def test_python_helper_agrees_with_c(rows):
    for of, nf, old, new, has_nil, nil_id, kind in rows:
        got = nif.classify_diffs([old], [new], [of * 1 + nf * 2], nil_id if has_nil else None)
        assert got == [kind], (of, nf, old, new, has_nil, nil_id)
    # and as one call over the rows that share a nil id
    many = [r for r in rows if r[4]]
    got = nif.classify_diffs([r[2] for r in many], [r[3] for r in many], [r[0] + 2 * r[1] for r in many],
                             many[0][5])
    assert got == [r[6] for r in many]
    assert nif.classify_diffs([], [], [], None) == []


def test_known_answers():
    """causal_crdt.ex:368-374 by hand: nil id 9, values 5 and 6."""
    OLD, NEW = 1, 2
    c = lambda o, n, f, nil=9: nif.classify_diffs([o], [n], [f], nil)[0]  # noqa: E731
    assert c(5, 5, OLD | NEW) == nif.DIFF_NONE          # {old, old}
    assert c(5, 6, OLD | NEW) == nif.DIFF_ADD           # {_, new}
    assert c(0, 6, NEW) == nif.DIFF_ADD                 # a new key
    assert c(5, 0, OLD) == nif.DIFF_REMOVE              # {_old, nil}: the key went
    assert c(5, 9, OLD | NEW) == nif.DIFF_REMOVE        # ... or its value became nil
    assert c(9, 5, OLD | NEW) == nif.DIFF_ADD           # nil before reads as absent
    assert c(9, 0, OLD) == nif.DIFF_NONE                # {nil, nil}
    assert c(0, 9, NEW) == nif.DIFF_NONE
    assert c(0, 0, 0) == nif.DIFF_NONE
    assert c(9, 9, OLD | NEW, nil=None) == nif.DIFF_NONE  # nil never interned: 9 is a value
    assert c(5, 9, OLD | NEW, nil=None) == nif.DIFF_ADD


def test_value_find_does_not_intern():
    U = interning.Universe()
    assert U.value_find(None) is None and U.value_find("v") is None and U.value_count() == 0
    assert U.value_find(1) == (1 << 62) + 1  # a canonical integer: closed form
    v, f = U.value("v"), U.value(1.0)
    assert U.value_find("v") == v and U.value_find(1.0) == f and f != U.value_find(1)
    assert U.value_find(Atom("x")) is None and U.value_count() == 2
    nil = U.value(None)
    assert U.value_find(None) == nil and U.value_count() == 3
