"""The inputs of tests/test_gpu_mutate_home.py (dg_mutate_home[_diffs]), built from per-key
recipes and checked on the CPU with the C oracle alone (test_mutate_home_cases.py) before
anything runs on a GPU: every case contains by construction what it is for, so a wrong kernel
cannot hide behind inputs that never ask.

A case is a state (its context a VV), a node and a batch of ops by that node.  A recipe gives
one key's state rows and its ops; the batch takes the recipes' ops round robin -- op 0 of
every key, then op 1 of every key, ... -- and the keys are random ids, so batch order is not
key order and an add's rank is not its position among its key's ops.  What the call must give
is the oracle's: mutate_batch (the delta, its dot list, the touched keys) -> join2 with the
touched keys -> changed_keys, and read/2 before and after (lww_diffs_cases.expected_diffs).

Recipes (state rows (val, ts, node) -> ops; the background keys' rows are by nodes 2 and 3):
  absent_add     nothing -> add (52, 9).                      A row comes: rows move.
  update1        (53, 7, 0) -> add (70, 9).                   1 -> 1: in place.
  update3        rows by nodes 0, 2, 3 -> add (71, 9).        3 -> 1: rows move.
  remove         (51, 7, 0) -> remove.                        1 -> 0.
  absent_remove  nothing -> remove.                           Touched, not changed.
  aa ar ra rr    (55, 7, 0) -> every (earlier, last) pair of add / remove.  aa's and ar's first
                 add is overwritten and its rank consumed all the same.
  neg_new        (56, 7, 2) -> add (57, -3): the new row's ts is negative, the old one's not.
  neg_old        (58, -7, 2) -> add (59, 3): the other way round.
  same_value     (54, 7, 0) -> add (54, 9): removed and re-added: an unchanged read.
  uncovered      (60, 7, 4) with dot (4, 100) while the VV has no node 4 -> add (61, 9): the
                 taken row's dot must reach the union context.
  in_both        a state row equal in all five columns to the row its add makes -- dot
                 (node, C[node] + 1 + rank), which the state's VV does not cover -> the add.  The
                 row is in both sides: it stays, the key does not change.
  deepN          N rows (1000 + i, 1) by nodes 2 and 3 -> add (5, 2).
  deepN_r        the same -> remove.
  addN           nothing -> N adds (the values differ).       N ops on one key.
"""
import numpy as np

from oracle import ref as R

# dg_mutate_home's limits (deltagpu.h)
MAX_OPS, MAX_TAKEN, MAX_NODES = 512, 1024, 2048

A, RM = "add", "remove"


def _recipe(name):
    """(state rows [(val, ts, node)], ops [(kind, val, ts)])"""
    if name.startswith("deep"):
        rm = name.endswith("_r")
        n = int(name[4:-2] if rm else name[4:])
        rows = [(1000 + i, 5 if i == n - 1 else 1, 2 + i % 2) for i in range(n)]
        return rows, [(RM, 0, 0)] if rm else [(A, 5, 2)]
    if name.startswith("add"):
        return [], [(A, 200 + i, 9 + i) for i in range(int(name[3:]))]
    return {
        "absent_add": ([], [(A, 52, 9)]),
        "update1": ([(53, 7, 0)], [(A, 70, 9)]),
        "update3": ([(40, 7, 0), (41, 8, 2), (42, 6, 3)], [(A, 71, 9)]),
        "remove": ([(51, 7, 0)], [(RM, 0, 0)]),
        "absent_remove": ([], [(RM, 0, 0)]),
        "aa": ([(55, 7, 0)], [(A, 80, 9), (A, 81, 10)]),
        "ar": ([(55, 7, 0)], [(A, 82, 9), (RM, 0, 0)]),
        "ra": ([(55, 7, 0)], [(RM, 0, 0), (A, 83, 9)]),
        "rr": ([(55, 7, 0)], [(RM, 0, 0), (RM, 0, 0)]),
        "neg_new": ([(56, 7, 2)], [(A, 57, -3)]),
        "neg_old": ([(58, -7, 2)], [(A, 59, 3)]),
        "same_value": ([(54, 7, 0)], [(A, 54, 9)]),
        "uncovered": ([(60, 7, 4)], [(A, 61, 9)]),
        "in_both": ([], [(A, 62, 9)]),  # (its state row is made from the add's dot, below)
    }[name]


def _sorted_rows(k, v, t, n, c):
    k, v = np.asarray(k, np.uint64), np.asarray(v, np.uint64)
    t, n, c = np.asarray(t, np.int64), np.asarray(n, np.uint32), np.asarray(c, np.uint64)
    o = np.lexsort((c, n, t, v, k))  # store order: key, {val, ts} (ts signed), dot
    return k[o], v[o], t[o], n[o], c[o]


def build(recipes, n_state=3000, node=5, node_in_vv=True, seed=0, key_bits=63):
    """The state {"rows", "ctx"}, the ops in batch order [(kind, key, val, ts)] and each
    recipe's key, for one key per entry of `recipes` among n_state one-row background keys.
    key_bits: the key ids are below 2^key_bits (62: all in shard 0 of a 2-bit shard tree)."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(1, 1 << key_bits, n_state + len(recipes) + 64, dtype=np.uint64))
    keys = rng.permutation(keys)[: n_state + len(recipes)]
    special, back = keys[: len(recipes)], keys[len(recipes):]  # (special: NOT sorted)
    cnt = {0: 0, 2: 0, 3: 0}
    c_node = 10 if node_in_vv else 0  # C[node]

    def dot(n):
        cnt[n] += 1
        return cnt[n]

    per_key = [_recipe(r) for r in recipes]
    ops, i = [], 0
    while any(i < len(o) for _, o in per_key):  # round robin: batch order is not key order
        for key, (_, o) in zip(special, per_key):
            if i < len(o):
                ops.append((o[i][0], int(key), o[i][1], o[i][2]))
        i += 1
    rank, r = {}, 0  # the rank of each key's LAST add
    for kind, key, _, _ in ops:
        if kind == A:
            rank[key] = r
            r += 1
    sk, sv, st, sn, sc = [], [], [], [], []
    for j, key in enumerate(back):
        n = 2 + j % 2
        sk.append(key), sv.append(int(rng.integers(1, 1 << 40))), st.append(7), sn.append(n), sc.append(dot(n))
    for key, name, (srows, _) in zip(special, recipes, per_key):
        for val, ts, n in srows:
            c = 100 if n == 4 else dot(n)
            sk.append(key), sv.append(val), st.append(ts), sn.append(n), sc.append(c)
        if name == "in_both":
            sk.append(key), sv.append(62), st.append(9), sn.append(node), sc.append(c_node + 1 + rank[int(key)])
    ents = [(n, c) for n, c in sorted(cnt.items()) if c > 0] + ([(node, c_node)] if node_in_vv else [])
    ents.sort()
    ctx = (R.VV, np.array([e[0] for e in ents], np.uint32), np.array([e[1] for e in ents], np.uint64))
    return {"rows": _sorted_rows(sk, sv, st, sn, sc), "ctx": ctx}, ops, special


EVERY = ["absent_add", "update1", "update3", "remove", "absent_remove", "aa", "ar", "ra", "rr", "neg_new",
         "neg_old", "same_value", "uncovered", "in_both"]
IN_PLACE = ["update1", "aa", "ra", "neg_new", "neg_old", "same_value", "in_both", "absent_remove"]

# name -> (recipes, state keys, node, node in the VV, served, rows move, what it must contain)
CASES = {
    # one key: a wave searches it, the tree's one-path case
    "one_absent_add": (["absent_add"], 3000, 5, True, True, True, ("added",)),
    "one_update1": (["update1"], 3000, 5, True, True, False, ("updated", "in_place")),
    "one_update3": (["update3"], 3000, 5, True, True, True, ("updated", "three_nodes")),
    "one_remove": (["remove"], 3000, 5, True, True, True, ("removed",)),
    "one_absent_remove": (["absent_remove"], 3000, 5, True, True, False, ("silent", "ctx_unchanged")),
    "one_same_value": (["same_value"], 3000, 5, True, True, False, ("unchanged_read",)),
    "one_in_both": (["in_both"], 3000, 5, True, True, False, ("in_both", "silent")),
    "one_uncovered": (["uncovered"], 3000, 5, True, True, False, ("uncovered",)),
    # every recipe: more than 8 keys, a thread searches each
    "every": (EVERY, 3000, 5, True, True, True,
              ("added", "updated", "removed", "silent", "rank_consumed", "pairs", "neg_ts", "unchanged_read",
               "uncovered", "in_both", "three_nodes")),
    "every_node_absent": (EVERY, 3000, 5, False, True, True, ("node_absent", "rank_consumed", "in_both")),
    "every_node70": (EVERY, 3000, 70, True, True, True, ("node70", "rank_consumed")),
    "node70_absent": (["absent_add", "aa"], 3000, 70, False, True, True, ("node70", "node_absent", "rank_consumed")),
    "node2047": (["absent_add", "update1"], 3000, 2047, True, True, True, ("node2047",)),
    "node2048": (["absent_add", "update1"], 3000, 2048, False, False, None, ("node2048",)),
    # a few keys (a wave each), every one keeping its row count: the in-place write
    "in_place": (IN_PLACE, 3000, 5, True, True, False, ("in_place", "silent", "rank_consumed")),
    "in_place_one_moves": (IN_PLACE + ["absent_add"], 3000, 5, True, True, True, ("added", "one_moves")),
    # the state's sizes around wave_find's window
    "state0": (["absent_add", "absent_remove"], 0, 5, True, True, True, ("added", "silent")),
    "state1": (["absent_add", "absent_remove"], 1, 5, True, True, True, ("added",)),
    "state64": (["absent_add", "absent_remove"] + ["update1"] * 3, 61, 5, True, True, True, ("added", "updated")),
    "state65": (["absent_add", "absent_remove"] + ["update1"] * 3, 62, 5, True, True, True, ("added", "updated")),
    # above 131,072 rows the moved rows are spliced after the wait
    "large_state": (EVERY, 140_000, 5, True, True, True, ("added", "removed", "large")),
    # the limits: 512 ops on 512 keys and on 3; one op more
    "ops512": ((["absent_add", "update1", "remove", "absent_remove"] * 128), 3000, 5, True, True, True,
               ("added", "updated", "removed", "silent", "ops512")),
    "ops513": ((["absent_add", "update1", "remove", "absent_remove"] * 128) + ["absent_add"], 3000, 5, True, False,
               None, ("ops513",)),
    "ops512_keys3": (["add170", "add171", "add171"], 3000, 5, True, True, True, ("ops512", "keys3", "rank_consumed")),
    # 1,024 state rows under the touched keys (16 keys of 64), each replaced by an add: the dot
    # list would have 1,040 dots, past the home join's 1,024; one row more is declined
    "taken1024": (["deep64"] * 16, 3000, 5, True, True, True, ("taken1024", "dots_over_1024")),
    "taken1025": (["deep64"] * 15 + ["deep65"], 3000, 5, True, False, None, ("taken1025",)),
}
ONE_KEY = [n for n in CASES if n.startswith("one_")]


def case(name, key_bits=63):
    recipes, n_state, node, in_vv, served, moves, must = CASES[name]
    a, ops, keys = build(recipes, n_state, node, in_vv, seed=len(name) + 7 * len(recipes), key_bits=key_bits)
    return {"name": name, "a": a, "ops": ops, "node": node, "keys": keys, "recipes": recipes, "served": served,
            "moves": moves, "must": must}


def marshal(ops):
    """dg_mutate_batch's arrays: the ops stably sorted by key, each add's rank in batch order."""
    kind = np.array([1 if o[0] == A else 0 for o in ops], np.uint8)
    key = np.array([o[1] for o in ops], np.uint64)
    val = np.array([o[2] for o in ops], np.uint64)
    ts = np.array([o[3] for o in ops], np.int64)
    rank = (np.cumsum(kind, dtype=np.uint64) - kind).astype(np.uint64)
    o = np.argsort(key, kind="stable")
    return kind[o], key[o], val[o], ts[o], rank[o], int(kind.sum())


def oracle(c):
    """The oracle's answer: the joined rows and context, the touched and the changed keys,
    read/2 of the changed keys before and after, and the delta the ops make."""
    from lww_diffs_cases import expected_diffs
    a = c["a"]
    dr, dc, touched = R.mutate_batch(a["rows"], a["ctx"], c["node"], c["ops"])
    wr, wc = R.join2(a["rows"], a["ctx"], dr, dc, keys=touched)
    wch = R.changed_keys(a["rows"], wr, touched)
    return {"rows": wr, "ctx": wc, "touched": touched, "changed": wch, "diffs": expected_diffs(a["rows"], wr, wch),
            "delta": dr, "dots": dc}
