"""The inputs of tests/test_gpu_mutate_seams.py (dg_mutate_batch, csrc/mutate.hip), built from
per-key recipes and checked on the CPU with the oracle alone (test_mutate_batch_cases.py)
before anything runs on a GPU: every case contains by construction what it is for, so a wrong
kernel cannot hide behind inputs that never ask.

A case is a state (rows and a VV), a node and the ops in batch order.  A group is one key's
state rows and its ops; the groups are given in KEY order (group j gets the j-th smallest of
the case's random key ids, all below 2^63), so a case says which sorted positions its ops
take, and the batch takes the groups' ops round robin over a random permutation of the groups
-- op 0 of every key, then op 1 of every key, ... -- so batch order is not key order and an
add's rank is not its position.  The arrays are mutate_home_cases.marshal's; what the call must
give is ref.mutate_batch's delta, dot list and touched keys, and ref.join2 with the touched
keys.  The background is 3,000 untouched keys of 1 to 3 rows each unless a case says otherwise.

The constants are mutate.hip's: TILE ops per tile (one workgroup), ROUND tiles per round of
the last tile's offset scan, GEN_PASS generated dots per pass of the generator's grid.

Seams (sorted positions):
  m255 m256 m257        one op per key: present and absent keys, adds and removes.
  m512_full             two tiles to the brim; the last group (3 ops) ends at op 511.
  ends_at_seam          a 3-op group at 253..255, the next group's head at 256.
  straddle_add_remove   a group at 254..257, ops add add remove remove: the last op in its
                        head's tile is an add, its last op (next tile) a remove.
  straddle_remove_add   the same key and positions, remove remove add add.
  group600              100 keys, then one key (3 state rows) with 600 ops at 100..699 (tile 1
                        holds no head) whose last op is an add, then 100 keys.
  extremes              300 one-op keys; at 250..255 and again at 256..261 adds with ts
                        INT64_MIN, -1, 0, INT64_MAX and val 0, 2^64 - 1.
Scan rounds and the generator's grid (ops drawn over 20,000 state keys and absent keys):
  tiles256 tiles257     65,536 and 65,537 ops, about 4 adds to 1 remove.
  tiles1025             262,400 ops, 200 of them removes: five rounds, more adds than GEN_PASS.
Dot-list paths:
  empty_state           no rows, a VV of no entries.
  all_absent            ops on absent keys only: below the first state key, above the last,
                        between two neighbours.  No state dots: the adds' dots are not sorted.
  removes_absent_only   touched keys, an empty delta, an empty dot list.
  removes_only          removes of present multi-row keys: a sort with nothing generated.
  vv_first vv_last vv_middle vv_single      the node's place in the VV (C[node] differs).
  vv_below vv_between vv_above              the node absent from it.
  wide_dots             node ids up to 2^31 and counters up to 2^64 - 2 under the touched keys;
                        the node is 65,536 with C[node] = 2^40 and has rows on both sides of
                        the dots it generates.
  long_runs             the store's first key has 1,025 rows (an add), its last 5,000 (a remove).
  many_rows_few_ops     3 removes on keys of 40 rows: 120 dots > 8 * 3 + 0 + 1, the wrappers'
                        first dot capacity.
  own_dot               state rows that carry the dot their key's add generates (mutate_home's
                        in_both): the kernel lists such a dot twice, the oracle's set once.
"""
import numpy as np

from mutate_home_cases import A, RM, _sorted_rows, marshal  # noqa: F401  (marshal: for the tests)
from oracle import ref as R

TILE, ROUND, GEN_PASS = 256, 256, 262_144
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
OWN = "own"  # a state row's counter: the dot of its key's last add


def _rows(k, nodes=(2, 3), base=900):
    """k state rows of one key, by `nodes` in turn; the counters are assigned by build()"""
    return [(base + i, 7 + i, nodes[i % len(nodes)], None) for i in range(k)]


def _draw_keys(rng, n):
    keys = np.unique(rng.integers(1, 1 << 63, n + 64, dtype=np.uint64))
    assert len(keys) >= n
    return np.sort(rng.permutation(keys)[:n])


def build(groups, n_back=3000, node=5, c_node=10, back_nodes=(2, 3), seed=0, place=None):
    """groups: [(state rows [(val, ts, node, cnt | None | OWN)], ops [(kind, val, ts)])] in key
    order.  c_node: C[node], None for a node absent from the VV (unless it has rows of its own
    with assigned counters).  place(background keys ascending) -> the groups' keys, where a
    case needs them somewhere in particular.  Returns the state {"rows", "ctx"}, the ops in
    batch order [(kind, key, val, ts)] and the groups' keys ascending."""
    rng = np.random.default_rng(seed)
    allk = _draw_keys(rng, n_back + len(groups))
    pick = np.zeros(len(allk), bool)
    pick[rng.choice(len(allk), len(groups), replace=False)] = True
    back = allk[~pick]
    special = allk[pick] if place is None else np.asarray(place(back), np.uint64)
    assert len(special) == len(groups) and np.all(special[1:] > special[:-1]) and not np.isin(special, back).any()
    # the batch: round robin over a permutation of the groups
    order = rng.permutation(len(groups))
    ops, i = [], 0
    longest = max((len(o) for _, o in groups), default=0)
    while i < longest:
        for j in order:
            o = groups[j][1]
            if i < len(o):
                ops.append((o[i][0], int(special[j]), o[i][1], o[i][2]))
        i += 1
    rank, r = {}, 0  # the rank of each key's LAST add
    for kind, key, _, _ in ops:
        if kind == A:
            rank[key] = r
            r += 1
    cnt = {}

    def dot(n):
        cnt[n] = cnt.get(n, 0) + 1
        return cnt[n]

    sk, sv, st, sn, sc = [], [], [], [], []
    n_rows = 1 + rng.integers(0, 3, len(back))
    vals = rng.integers(1, 1 << 40, int(n_rows.sum()))
    q = 0
    for j, key in enumerate(back):
        for i in range(int(n_rows[j])):
            n = back_nodes[(j + i) % len(back_nodes)]
            sk.append(key), sv.append(int(vals[q])), st.append(7 + i), sn.append(n), sc.append(dot(n))
            q += 1
    for key, (srows, _) in zip(special, groups):
        for val, ts, n, c in srows:
            if c is None:
                c = dot(n)
            elif c == OWN:
                c = c_node + 1 + rank[int(key)]
            sk.append(key), sv.append(val), st.append(ts), sn.append(n), sc.append(c)
    vv = dict(cnt)
    if c_node is not None:
        vv[node] = max(c_node, vv.get(node, 0))
    ents = sorted(vv.items())
    ctx = (R.VV, np.array([e[0] for e in ents], np.uint32), np.array([e[1] for e in ents], np.uint64))
    return {"rows": _sorted_rows(sk, sv, st, sn, sc), "ctx": ctx}, ops, special


def drawn(m, n_removes, seed, n_state=20_000, node=5, c_node=10):
    """m ops drawn over n_state state keys (1 to 3 rows each) and, one time in five, a key of
    its own; n_removes of them removes, at random places."""
    rng = np.random.default_rng(seed)
    a, _, _ = build([], n_back=n_state, node=node, c_node=c_node, seed=seed)
    skeys = np.unique(a["rows"][0])
    key = skeys[rng.integers(0, len(skeys), m)]
    fresh = rng.random(m) < 0.2
    key[fresh] = rng.integers(1, int(skeys[-1]), int(fresh.sum()), dtype=np.uint64)
    add = np.ones(m, bool)
    add[rng.choice(m, n_removes, replace=False)] = False
    # the last sorted op is a group of its own, an add on the state's last key: where it is
    # alone in its tile (tiles257) that tile still counts a key, a row and state dots
    key[key == skeys[-1]] = skeys[0]
    at = int(rng.integers(0, m))
    key[at], add[at] = skeys[-1], True
    val = rng.integers(1, 1 << 62, m, dtype=np.uint64)
    ts = rng.integers(-(1 << 40), 1 << 40, m)
    ops = [(A, k, v, t) if x else (RM, k, 0, 0) for x, k, v, t in zip(add.tolist(), key.tolist(), val.tolist(), ts.tolist())]
    return a, ops, np.zeros(0, np.uint64)


# ---------------------------------------------------------------- groups

def _add(i, ts=None):
    return (A, 5000 + i, 9 + i if ts is None else ts)


_RM = (RM, 0, 0)


def _single(i):
    """one op on one key: present / absent, add / remove in turn; 1 to 3 state rows"""
    return [(_rows(1 + i % 3), [_add(i)]), ([], [_add(i, -3 - i)]), (_rows(1 + (i // 4) % 3), [_RM]), ([], [_RM])][i % 4]


def _singles(n, start=0):
    return [_single(start + i) for i in range(n)]


def _mixed(n):
    """n keys of 0 to 3 state rows and 1 to 3 ops, every (earlier, last) pair among them"""
    pats = [[_add], [RM], [_add, _add], [_add, RM], [RM, _add], [RM, RM], [_add, RM, _add]]
    out = []
    for i in range(n):
        ops = [_RM if f is RM else f(10 * i + q) for q, f in enumerate(pats[i % len(pats)])]
        out.append((_rows((i // len(pats)) % 4), ops))
    return out


def _straddle(first):
    second = RM if first == A else A
    four = [_add(900 + q) if k == A else _RM for q, k in enumerate((first, first, second, second))]
    return _singles(254) + [(_rows(2), four)] + _singles(40, 254)


def _group600():
    ops = [_add(1000 + q) if q % 3 else _RM for q in range(599)] + [_add(1599)]
    return _singles(100) + [(_rows(3), ops)] + _singles(100, 100)


def _extremes():
    ext = [(A, 6000, I64_MIN), (A, 6001, -1), (A, 6002, 0), (A, 6003, I64_MAX), (A, 0, 11), (A, U64_MAX, 12)]
    side = [(_rows(i % 3), [op]) for i, op in enumerate(ext)]  # (absent, one row, two rows in turn)
    return _singles(250) + side + side + _singles(38, 250)


WIDE_NODES = [0, 1, 255, 256, 65_535, 65_536, 1 << 24, 1 << 31]
WIDE_CNTS = [1, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 48, 1 << 63, (1 << 64) - 2]
WIDE_NODE, WIDE_C = 65_536, 1 << 40


def _wide():
    """every (node, counter) pair of the two lists as a state row, three to a touched key"""
    pairs = [(n, c) for c in WIDE_CNTS for n in WIDE_NODES]
    out = []
    for j in range(0, len(pairs), 3):
        rows = [(700 + j + i, 7 + i, n, c) for i, (n, c) in enumerate(pairs[j:j + 3])]
        out.append((rows, [_add(j)] if (j // 3) % 2 == 0 else [_RM]))
    return out + [([], [_add(500 + i)]) for i in range(10)]


def _absent_places(n):
    """below the first state key, between neighbours, above the last"""
    def place(back):
        assert int(back[0]) > 1 and int(back[-1]) < (1 << 63) - 1
        at = np.linspace(0, len(back) - 2, n - 2).astype(int)
        assert len(set(at.tolist())) == n - 2 and np.all(back[at + 1] - back[at] > 1)
        return np.concatenate([[back[0] // np.uint64(2)], back[at] + (back[at + 1] - back[at]) // np.uint64(2),
                               [back[-1] + (np.uint64(1 << 63) - back[-1]) // np.uint64(2)]])
    return place


def _long_runs_places(back):
    return np.array([back[0] // np.uint64(2), back[-1] + (np.uint64(1 << 63) - back[-1]) // np.uint64(2)], np.uint64)


def _long(k):
    return [(10_000 + i, i - 100, 2 + i % 2, None) for i in range(k)]


def _own():
    own = lambda i: ([(5000 + i, 9 + i, 5, OWN)], [_add(i)])  # noqa: E731  (the row its add makes)
    g = _singles(40)
    for at, i in ((3, 100), (17, 101), (30, 102)):
        g.insert(at, own(i))
    return g


# name -> (groups, build's other arguments)
CASES = {
    "m255": (lambda: _singles(255), {}),
    "m256": (lambda: _singles(256), {}),
    "m257": (lambda: _singles(257), {}),
    "m512_full": (lambda: _singles(509) + [(_rows(2), [_add(600), _RM, _add(601)])], {}),
    "ends_at_seam": (lambda: _singles(253) + [(_rows(2), [_RM, _add(700), _add(701)]), (_rows(1), [_add(702), _RM])]
                     + _singles(42, 253), {}),
    "straddle_add_remove": (lambda: _straddle(A), {}),
    "straddle_remove_add": (lambda: _straddle(RM), {}),
    "group600": (_group600, {}),
    "extremes": (_extremes, {}),
    "empty_state": (lambda: [([], o) for _, o in _mixed(40)], {"n_back": 0, "c_node": None}),
    "all_absent": (lambda: [([], o) for _, o in _mixed(30)], {"place": _absent_places(30)}),
    "removes_absent_only": (lambda: [([], [_RM] * (1 + i % 2)) for i in range(20)], {}),
    "removes_only": (lambda: [(_rows(2 + i % 3), [_RM] * (1 + i % 2)) for i in range(40)], {}),
    "vv_first": (lambda: _mixed(60), {"node": 1, "c_node": 10}),
    "vv_last": (lambda: _mixed(60), {"node": 9, "c_node": 1000}),
    "vv_middle": (lambda: _mixed(60), {"node": 5, "c_node": 77, "back_nodes": (2, 7)}),
    "vv_below": (lambda: _mixed(60), {"node": 1, "c_node": None}),
    "vv_between": (lambda: _mixed(60), {"node": 5, "c_node": None, "back_nodes": (2, 7)}),
    "vv_above": (lambda: _mixed(60), {"node": 9, "c_node": None}),
    # one entry, the node's own: its earlier writes are the state
    "vv_single": (lambda: [(_rows(len(r), (5,)), o) for r, o in _mixed(60)], {"node": 5, "c_node": None,
                                                                               "back_nodes": (5,)}),
    "wide_dots": (_wide, {"node": WIDE_NODE, "c_node": WIDE_C}),
    "long_runs": (lambda: [(_long(1025), [_add(1)]), (_long(5000), [_RM])], {"place": _long_runs_places}),
    "many_rows_few_ops": (lambda: [(_rows(40), [_RM])] * 3, {}),
    "own_dot": (_own, {}),
}
# name -> (ops, removes among them)
DRAWN = {"tiles256": (ROUND * TILE, 13_000), "tiles257": (ROUND * TILE + 1, 13_000), "tiles1025": (1025 * TILE, 200)}
SEAMS = ["m255", "m256", "m257", "m512_full", "ends_at_seam", "straddle_add_remove", "straddle_remove_add",
         "group600", "extremes"]
NAMES = SEAMS + list(DRAWN) + [n for n in CASES if n not in SEAMS]
SEED = 11  # one seed: straddle_add_remove and straddle_remove_add share their keys


def case(name):
    if name in DRAWN:
        m, n_removes = DRAWN[name]
        a, ops, keys = drawn(m, n_removes, SEED + m % 7)
        node = 5
    else:
        groups, kw = CASES[name]
        a, ops, keys = build(groups(), seed=SEED, **kw)
        node = kw.get("node", 5)
    return {"name": name, "a": a, "ops": ops, "node": node, "keys": keys}


def oracle(c, join=True):
    """ref.mutate_batch's delta, dot list and touched keys, and ref.join2's rows and context"""
    a = c["a"]
    dr, dc, touched = R.mutate_batch(a["rows"], a["ctx"], c["node"], c["ops"])
    o = {"delta": dr, "dots": dc, "touched": touched}
    if join:
        o["rows"], o["ctx"] = R.join2(a["rows"], a["ctx"], dr, dc, keys=touched)
    return o
