"""The calls of tests/inplace_cases.py are what they claim to be: on the C oracle's keyed join
every keyset key keeps its row count, and a plain restatement of dg_kdw.h's in-place write
loop (naive_in_place) gets the named multi-row keys and a fair share of the random ones wrong
-- so tests/test_gpu_inplace_multirow.py passing on a case means the kernel did not read back
a row it had just written.  No GPU.

Measured on the oracle (seed 11, the same for both context kinds and both node ranges): 47
keys bite -- front, middle, two, wide and 43 of the 150 random keys -- in count tiles 0, 1 and
2 (20, 21 and 6 keys), 33 of them with a row the delta holds too; 107 random keys, back,
pair, shared, one and all 442 filler keys do not.  reads_back, the count kernel's rule for
leaving the in-place path, names the same 47 keys."""
import numpy as np
import pytest

import inplace_cases as IC
from oracle import ref as R

KINDS = [IC.VV, IC.DOTS]
BASES = [IC.KVT - 4, IC.KVT]  # nodes 1020..1023 (the LDS tables' last entries) and 1024..1027


def counts(rows, keys):
    return np.searchsorted(rows[0], keys, "right") - np.searchsorted(rows[0], keys, "left")


def test_naive_in_place_is_the_write_loop():
    """The advice's example by hand: [X, Y, Z] -> [D, X, Y] leaves [D, X, X]; the harmless
    direction [Z, X, Y] -> [X, Y, D'] and a two-row key come out right."""
    k = 7
    X, Y, Z, D, E = (k, 20, 0, 1, 1), (k, 30, 0, 1, 2), (k, 40, 0, 2, 1), (k, 10, 0, 3, 1), (k, 50, 0, 3, 2)
    st = IC.rows_from([X, Y, Z])
    assert IC.naive_in_place(st, IC.rows_from([D, X, Y]), k) == [D, X, X]
    assert IC.naive_in_place(IC.rows_from([D, X, Y]), IC.rows_from([X, Y, E]), k) == [X, Y, E]
    assert IC.naive_in_place(IC.rows_from([X, Z]), IC.rows_from([D, X]), k) == [D, X]
    assert IC.naive_in_place(st, st, k) == [X, Y, Z]


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("kind", KINDS)
def test_count_preserving_case_bites(kind, base):
    c = IC.case(kind, base)
    st, d, keys = c["state"], c["delta"], c["keys"]
    assert len(keys) == IC.N_KEYSET == 2 * IC.KD_BLOCK + 88 and st["ctx"][0] == IC.VV and d["ctx"][0] == kind
    assert len(np.unique(st["rows"][0])) == IC.N_KEYS and R.store_check(st["rows"]) and R.store_check(d["rows"])
    assert np.isin(d["rows"][0], keys).all()  # sync-shaped: no delta row outside the keyset
    na = counts(st["rows"], np.unique(st["rows"][0]))
    assert na.min() == 1 and np.median(na) in (4, 5) and np.sort(na)[-2] <= 12 and na.max() == IC.KD_RUN
    nodes = np.unique(np.concatenate([st["rows"][3], d["rows"][3]]))
    assert (nodes < IC.KVT).all() if base < IC.KVT else (nodes >= IC.KVT).all()
    for name, (pos, *_) in IC.NAMED.items():
        assert keys[pos] == c["named"][name]
    assert {IC.NAMED[n][0] for n in ("front", "middle", "two", "wide")} == {0, 255, 256, 599}
    want, _ = IC.joined(c)
    assert np.array_equal(counts(st["rows"], keys), counts(want, keys))  # every key keeps its count
    changed = set(R.changed_keys(st["rows"], want, keys).tolist())
    assert changed == set(c["named"].values()) | set(c["random"])
    # each named key's rows, as the module's table says
    for name, (_, n, removed, gaps, shared) in IC.NAMED.items():
        old, new = IC.key_rows(st["rows"], c["named"][name]), IC.key_rows(want, c["named"][name])
        assert len(old) == len(new) == n
        kept = [r for i, r in enumerate(old) if i not in removed]
        assert [r for r in new if r in old] == kept and len(set(new) - set(old)) == len(gaps)
        held = IC.key_rows(d["rows"], c["named"][name])
        assert [r for r in old if r in held] == [old[i] for i in shared]
    f, o = IC.key_rows(want, c["named"]["front"]), IC.key_rows(st["rows"], c["named"]["front"])
    assert f[0] < o[0] and f[1:] == o[:2]  # [X, Y, Z] -> [D, X, Y], D < X
    b = set(IC.bites(c))
    for name in IC.BITING:
        assert c["named"][name] in b, name
    for name in IC.HARMLESS:
        assert c["named"][name] not in b, name
    assert not b & set(c["filler"])
    # the count kernel's rule for leaving the in-place path names exactly these keys
    assert [int(x) for x in keys if IC.reads_back(st["rows"], want, x)] == sorted(b)
    hit = [x for x in c["random"] if x in b]
    assert len(hit) >= 40 and len(c["random"]) - len(hit) >= 40, (len(hit), len(c["random"]))
    assert {int(np.searchsorted(keys, x)) // IC.KD_BLOCK for x in b} == {0, 1, 2}
    # the delta also holds rows the state keeps (the `same row` branch), some of them in keys that bite
    both = [x for x in c["random"] if set(IC.key_rows(d["rows"], x)) & set(IC.key_rows(st["rows"], x))]
    assert len(both) >= 20 and len(set(both) & b) >= 5


@pytest.mark.parametrize("kind", KINDS)
def test_quiet_changes_one_row_keys_only(kind):
    c, h = IC.case(kind, 0, "quiet"), IC.case(kind, 0)
    assert all(np.array_equal(x, y) for x, y in zip(c["state"]["rows"], h["state"]["rows"]))
    assert np.array_equal(c["keys"], h["keys"])
    want, _ = IC.joined(c)
    assert R.changed_keys(c["state"]["rows"], want, c["keys"]).tolist() == [c["named"]["one"]]
    assert np.array_equal(counts(c["state"]["rows"], c["keys"]), counts(want, c["keys"]))
    assert (counts(c["state"]["rows"], c["keys"]) > 1).sum() > 400 and IC.bites(c) == []
    assert not any(IC.reads_back(c["state"]["rows"], want, x) for x in c["keys"])
    # the delta still holds rows of unchanged multi-row keys
    assert len(np.unique(c["delta"]["rows"][0])) > 50


@pytest.mark.parametrize("variant", ["one_moves", "outside"])
def test_variants_with_an_added_key(variant):
    c, h = IC.case(IC.VV, 0, variant), IC.case(IC.VV, 0)
    x = c["extra"]
    assert len(c["keys"]) == IC.N_KEYSET + 1 and x in c["keys"] and x not in h["keys"]
    want, _ = IC.joined(c)
    ch = set(R.changed_keys(c["state"]["rows"], want, c["keys"]).tolist())
    assert ch == set(c["named"].values()) | set(c["random"]) | {x}
    moved = counts(c["state"]["rows"], c["keys"]) != counts(want, c["keys"])
    if variant == "one_moves":
        assert c["keys"][moved].tolist() == [x] and IC.key_rows(c["state"]["rows"], x) == []
    else:
        assert not moved.any() and x >> 63 == 1 and (h["keys"] >> np.uint64(63) == 0).all()
        assert len(IC.key_rows(c["state"]["rows"], x)) == 1 and x not in IC.bites(c)
    assert set(IC.bites(c)) == set(IC.bites(h))


@pytest.mark.parametrize("kind", KINDS)
def test_named_keys_alone(kind):
    """Each named key as a call of its own gives the key the rows the whole call gives it."""
    c = IC.case(kind, 0)
    whole, _ = IC.joined(c)
    for name, x in c["named"].items():
        d, ks = IC.alone(c, name)
        assert ks.tolist() == [x] and set(d["rows"][0].tolist()) == {x} and d["ctx"][0] == kind
        got, _ = R.join2(c["state"]["rows"], c["state"]["ctx"], d["rows"], d["ctx"], keys=ks)
        assert IC.key_rows(got, x) == IC.key_rows(whole, x)
        assert R.changed_keys(c["state"]["rows"], got).tolist() == [x]
    d, _ = IC.alone(c, "front")
    assert len(d["rows"][0]) == 1 and len(d["ctx"][1]) == 2  # one row, two dots: the six-row reproducer
