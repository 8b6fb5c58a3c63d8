"""The inputs of tests/test_gpu_home_diffs.py (dg_join_delta_home_diffs), built from per-key
recipes so that every class of changed key of lww_diffs_cases.classes is present by
construction, and checked on the CPU with the C oracle alone (test_home_diffs_cases.py)
before anything runs on a GPU: a wrong winner cannot hide behind inputs that never ask for it.

A case is a state, a delta whose every key is in the keyset, and the keyset.  The state's
rows are by nodes 0..3 (its VV covers them), the delta's by node 5:
  * a state row by node 0 is COVERED by the delta's context and goes (unless the delta has it);
  * a state row by node 2 or 3 is kept: the delta's context names neither node;
  * a delta row by node 5 is new to the state and comes in;
  * the silent key's delta row is dot (1, 1): the state's VV covers it and no state row has
    it, so it is dropped and the key does not change.
The delta's context is the dot set of the covered dots and the delta's own, or -- `vv` -- the
VV {0: max, 1: 1, 5: max} that covers exactly the same state rows.

Recipes (state rows -> delta rows; (value, ts) pairs):
  unchanged  (50, 7) kept; + (60, 3): a new dot under an older ts. Both flags, equal values.
  removed    (51, 7) covered; nothing comes.                         OLD only.
  added      nothing; + (52, 9).                                     NEW only.
  updated    (53, 7) covered; + (70, 9).                             In place: 1 row -> 1 row.
  tie        (20, 7) covered, (30, 7) kept; + (25, 7).  Two values at the maximal ts before
             (20 wins) and after (25 wins): updated, decided by the tie-break.  2 -> 2 rows.
  signed     (50, 4) kept, (60, -3) kept; + (55, -1).  The winner is decided across the sign:
             an unsigned compare would take ts -3.  Unchanged read.
  reappear   (54, 7) covered; + (54, 9): removed and re-added by one delta.  1 -> 1 row.
  silent     (56, 7) kept; + (99, 9) with dot (1, 1): dropped.  Not a changed key.
  keep2      (50, 7) kept, (40, 2) covered; + (60, 3): `unchanged` keeping its row count.
  signed3    `signed` plus (65, -8) covered: keeps its row count.
  deep(n)    n rows (1000 + i, 1) kept, the last one at ts 5: the winner is the LAST row
             walked; + (5, 2).  Unchanged read.

Which classes a case must hold (`must`): all five wherever the case's own shape allows it.
Two shapes do not: a keyset of ONE key holds one class (the five one-key cases hold the five
between them), and a case in which every key keeps its row count cannot remove or add a key.
"""
import numpy as np

from oracle import ref as R

ALL = ("unchanged", "removed", "added", "updated", "ties")
# dg_join_delta_home's limits (deltagpu.h)
MAX_KEYS, MAX_DELTA, MAX_DCTX, MAX_TAKEN, MAX_EDIT = 512, 512, 1024, 1024, 1536

CYCLE = ("unchanged", "removed", "added", "updated", "tie", "signed", "reappear", "silent")
IN_PLACE = ("keep2", "updated", "tie", "signed3", "reappear", "silent")


def _recipe(name):
    """(state rows [(val, ts, node)], delta rows [(val, ts)]; the silent key's delta dot is (1, 1))"""
    if name.startswith("deep"):
        n = int(name[4:])
        return [(1000 + i, 5 if i == n - 1 else 1, 2 + i % 2) for i in range(n)], [(5, 2)]
    return {
        "unchanged": ([(50, 7, 2)], [(60, 3)]),
        "removed": ([(51, 7, 0)], []),
        "added": ([], [(52, 9)]),
        "updated": ([(53, 7, 0)], [(70, 9)]),
        "tie": ([(20, 7, 0), (30, 7, 2)], [(25, 7)]),
        "signed": ([(50, 4, 2), (60, -3, 3)], [(55, -1)]),
        "reappear": ([(54, 7, 0)], [(54, 9)]),
        "silent": ([(56, 7, 3)], [(99, 9)]),
        "keep2": ([(50, 7, 2), (40, 2, 0)], [(60, 3)]),
        "signed3": ([(50, 4, 2), (60, -3, 3), (65, -8, 0)], [(55, -1)]),
    }[name]


def _sorted_rows(k, v, t, n, c):
    k, v = np.asarray(k, np.uint64), np.asarray(v, np.uint64)
    t, n, c = np.asarray(t, np.int64), np.asarray(n, np.uint32), np.asarray(c, np.uint64)
    o = np.lexsort((c, n, t, v, k))  # store order: key, {val, ts} (ts signed), dot
    return k[o], v[o], t[o], n[o], c[o]


def build(recipes, n_state=3000, vv=False, seed=0):
    """{"rows", "ctx"} of the state and of the delta, and the keyset (ascending), for one key
    per entry of `recipes` among `n_state` one-row background keys (nodes 2 and 3)."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1, 1 << 63, n_state + len(recipes) + 64, dtype=np.uint64))
    keys = rng.permutation(keys)[: n_state + len(recipes)]
    special, back = np.sort(keys[: len(recipes)]), keys[len(recipes):]
    cnt = {0: 0, 1: 1, 2: 0, 3: 0, 5: 0}  # node 1 starts at 2: dot (1, 1) is no state row

    def dot(node):
        cnt[node] += 1
        return cnt[node]

    sk, sv, st, sn, sc = [], [], [], [], []
    dk, dv, dt, dn, dc = [], [], [], [], []
    covered = []
    for i, key in enumerate(back):
        node = 2 + i % 2
        sk.append(key), sv.append(int(rng.integers(1, 1 << 40))), st.append(7), sn.append(node), sc.append(dot(node))
    for key, name in zip(special, recipes):
        srows, drows = _recipe(name)
        for val, ts, node in srows:
            c = dot(node)
            sk.append(key), sv.append(val), st.append(ts), sn.append(node), sc.append(c)
            if node == 0:
                covered.append((0, c))
        for val, ts in drows:
            node, c = (1, 1) if name == "silent" else (5, dot(5))
            dk.append(key), dv.append(val), dt.append(ts), dn.append(node), dc.append(c)
    state_ctx = (R.VV, np.arange(4, dtype=np.uint32), np.array([cnt[0], cnt[1], cnt[2], cnt[3]], np.uint64))
    if vv:
        ents = [(0, cnt[0]), (1, 1), (5, cnt[5])]
        ents = [e for e in ents if e[1] > 0 and (e[0] != 1 or "silent" in recipes)]
        kind = R.VV
    else:
        ents = sorted(set(covered) | {(int(n), int(c)) for n, c in zip(dn, dc)})
        kind = R.DOTS
    delta_ctx = (kind, np.array([e[0] for e in ents], np.uint32), np.array([e[1] for e in ents], np.uint64))
    return ({"rows": _sorted_rows(sk, sv, st, sn, sc), "ctx": state_ctx},
            {"rows": _sorted_rows(dk, dv, dt, dn, dc), "ctx": delta_ctx}, special)


def _cycle(n):
    return [CYCLE[i % len(CYCLE)] for i in range(n)]


# name -> (recipes, state keys, classes it must hold, falls back, rows move)
CASES = {
    # a few keys: one wave searches each (nk <= 8) ...
    "one_unchanged": (["unchanged"], 3000, ("unchanged",), False, True),
    "one_removed": (["removed"], 3000, ("removed",), False, True),
    "one_added": (["added"], 3000, ("added",), False, True),
    "one_updated": (["updated"], 3000, ("updated",), False, False),
    "one_tie": (["tie"], 3000, ("updated", "ties"), False, False),
    "keys8": (_cycle(8), 3000, ALL, False, True),
    # ... more: one thread searches each
    "keys9": (_cycle(8) + ["updated"], 3000, ALL, False, True),
    "keys512": (_cycle(512), 3000, ALL, False, True),
    # both write paths: every key keeps its row count / exactly one key's changes
    "in_place": (list(IN_PLACE) * 2, 3000, ("unchanged", "updated", "ties"), False, False),
    "one_key_moves": (list(IN_PLACE) * 2 + ["added"], 3000, ("unchanged", "added", "updated", "ties"), False, True),
    # above 131,072 rows the moved rows are spliced after the wait
    "large_state": (_cycle(8), 140_000, ALL, False, True),
    # 1,000 rows under one key, the winner the last row (1,004 taken rows of 1,024)
    "deep": (["deep1000", "removed", "added", "updated", "tie"], 3000, ALL, False, True),
    # 1,025: over the limit, nothing happens
    "deep_over": (["deep1025"], 3000, ("unchanged",), True, None),
}
ONE_KEY = ("one_unchanged", "one_removed", "one_added", "one_updated", "one_tie")


def case(name, vv=False):
    recipes, n_state, must, fallback, moves = CASES[name]
    a, d, keys = build(recipes, n_state, vv, seed=len(name) + 7 * len(recipes))
    return {"name": name, "a": a, "d": d, "keys": keys, "recipes": recipes, "must": must,
            "fallback": fallback, "moves": moves}


def oracle(c):
    """The oracle's join of a case, its changed keys, and what the three arrays must hold."""
    from lww_diffs_cases import classes, expected_diffs
    a, d, keys = c["a"], c["d"], c["keys"]
    wr, wc = R.join2(a["rows"], a["ctx"], d["rows"], d["ctx"], keys=keys)
    wch = R.changed_keys(a["rows"], wr, keys)
    want = expected_diffs(a["rows"], wr, wch)
    return wr, wc, wch, want, classes(wr, wch, *want)
