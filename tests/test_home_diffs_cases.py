"""The generator of the dg_join_delta_home_diffs cases (home_diffs_cases.py) checked with the
C oracle alone, no GPU: every case's changed keys hold the classes it must (all five of
lww_diffs_cases.classes wherever the case's shape allows), the cases the GPU test expects
the small path to take stay inside its limits, the one that must fall back is outside
them, and the rows move exactly where the case says."""
import numpy as np
import pytest

import home_diffs_cases as H
from lww_diffs_cases import NEW, OLD


def _run_lengths(rows, keys):
    return np.searchsorted(rows[0], keys, "right") - np.searchsorted(rows[0], keys, "left")


@pytest.mark.parametrize("vv", [False, True])
@pytest.mark.parametrize("name", list(H.CASES))
def test_case_holds_its_classes_and_limits(name, vv):
    c = H.case(name, vv)
    a, d, keys = c["a"], c["d"], c["keys"]
    wr, wc, wch, (ov, nv, fl), cls = H.oracle(c)
    for k in c["must"]:
        assert cls[k] >= 1, (name, cls)
    if name not in H.ONE_KEY and name not in ("in_place", "one_key_moves", "deep_over"):
        assert c["must"] == H.ALL
    # the keyset is the delta's keys plus keys the delta only removes from; sorted and unique
    assert np.all(np.diff(keys.astype(np.float64)) > 0) and len(keys) == len(c["recipes"])
    assert np.isin(d["rows"][0], keys).all()
    # a silent key is in the keyset and not among the changed keys; every other key changes
    silent = keys[[r == "silent" for r in c["recipes"]]]
    assert not np.isin(silent, wch).any()
    assert len(wch) == len(keys) - len(silent)
    # the limits of the small path (the delta's, the taken rows, the edit, node ids)
    taken = int(_run_lengths(a["rows"], keys).sum())
    edit = int(_run_lengths(wr, keys).sum())
    inside = (len(keys) <= H.MAX_KEYS and len(d["rows"][0]) <= H.MAX_DELTA and len(d["ctx"][1]) <= H.MAX_DCTX
              and taken <= H.MAX_TAKEN and edit <= H.MAX_EDIT and a["ctx"][0] == 0 and len(wc[1]) <= 2048)
    assert inside == (not c["fallback"]), (name, taken, edit)
    if c["fallback"]:
        assert taken == H.MAX_TAKEN + 1  # just over: 1,025 rows under the one key
    else:
        moved = bool((_run_lengths(a["rows"], keys) != _run_lengths(wr, keys)).any())
        assert moved == c["moves"], name
    if name == "one_key_moves":
        assert int((_run_lengths(a["rows"], keys) != _run_lengths(wr, keys)).sum()) == 1
    if name == "large_state":
        assert len(a["rows"][0]) > 131_072
    if name == "deep":
        assert _run_lengths(a["rows"], keys).max() == 1000 and taken <= H.MAX_TAKEN


def test_one_key_cases_hold_the_five_classes_between_them():
    seen = set()
    for name in H.ONE_KEY:
        c = H.case(name)
        assert len(c["keys"]) == 1
        cls = H.oracle(c)[4]
        seen |= {k for k, n in cls.items() if n}
    assert seen == set(H.ALL)


@pytest.mark.parametrize("vv", [False, True])
def test_recipes_read_what_they_say(vv):
    """Known answers for the recipes the GPU cases lean on (the walk's winner rule)."""
    c = H.case("keys8", vv)
    wr, wc, wch, (ov, nv, fl), cls = H.oracle(c)
    by = {r: (int(o), int(n), int(f)) for r, o, n, f in
          zip([r for r in c["recipes"] if r != "silent"], ov, nv, fl)}
    assert by["unchanged"] == (50, 50, OLD | NEW)
    assert by["removed"] == (51, 0, OLD)
    assert by["added"] == (0, 52, NEW)
    assert by["updated"] == (53, 70, OLD | NEW)
    assert by["tie"] == (20, 25, OLD | NEW)          # the smaller value at the maximal ts, twice
    assert by["signed"] == (50, 50, OLD | NEW)       # ts 4 beats ts -3 and -1
    assert by["reappear"] == (54, 54, OLD | NEW)
    d = H.case("deep", vv)
    ov, nv, fl = H.oracle(d)[3]
    i = d["recipes"].index("deep1000")
    assert (int(ov[i]), int(nv[i]), int(fl[i])) == (1999, 1999, OLD | NEW)  # the last row walked
    # both context kinds cover the same rows
    assert all(np.array_equal(x, y) for x, y in zip(wr, H.oracle(H.case("keys8", not vv))[0]))
