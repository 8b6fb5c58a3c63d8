"""The hops of a batch of continuations (dg_merkle_continues, dgr_merkle_continue_batch): what
one replica X has to answer in the conversations of tests/partial_diff_cases.py, from the C
oracle alone (helper module: no tests, no GPU).

A hop is (cont, want): the oracle's continuation X receives and what the oracle answers it
with on X's tree -- ("continue", cont') truncated to max_sync, or ("ok", keys)."""
import functools

import numpy as np

import partial_diff_cases as P
from oracle import ref as R


@functools.lru_cache(maxsize=None)
def oracle_tree(rows_id, depth, shard_bits=0, shard=0):
    return R.merkle_build(_ROWS[rows_id], depth, shard_bits, shard)


_ROWS: dict = {}


def tree_of(rows, depth, shard_bits=0, shard=0):
    """the oracle's tree over rows, built once per (rows, shape)"""
    _ROWS[id(rows[0])] = rows
    return oracle_tree(id(rows[0]), depth, shard_bits, shard)


def answer(tx, rows_x, rc, levels, max_sync):
    """the oracle's hop on X: continue_partial_diff, then truncate_diff"""
    res = R.merkle_continue(tx, rows_x, rc, levels)
    if res[0] == "continue" and max_sync is not None:
        res = ("continue", R.merkle_truncate(tx, res[1], max_sync))
    return res


def hops_of(rows_x, peers, depth, levels, max_sync, shard_bits=0, shard=0):
    """Every continuation X answers in its walks with each of `peers` (rows), both
    orientations (X prepares / the peer prepares), in conversation order."""
    tx = tree_of(rows_x, depth, shard_bits, shard)
    out = []
    for rows_p in peers:
        tp = tree_of(rows_p, depth, shard_bits, shard)
        for x_prepares in (False, True):
            first, second = ((None, tx, rows_x), (None, tp, rows_p)) if x_prepares else (
                (None, tp, rows_p), (None, tx, rows_x))
            conts = P.run_protocol(first, second, levels, max_sync)["conts"]
            # conts[i] is answered by `second` for even i, by `first` for odd i
            for i, rc in enumerate(conts):
                if (i % 2 == 1) == x_prepares:
                    out.append((rc, answer(tx, rows_x, rc, levels, max_sync)))
    return out


def kind_of(want):
    """the four result kinds: node out, leaf out, keys, empty ({:ok, []})"""
    if want[0] == "continue":
        return want[1][0]
    return "keys" if len(want[1]) else "empty"


_EMPTY = P.empty_rows()


@functools.lru_cache(maxsize=None)
def ladder_hops(max_sync=None, levels=3, shard_bits=0, shard=0):
    """X = the ladder's side A against its side B, an empty replica and itself."""
    a, b, _ = P.ladder(8, shard_bits, shard)
    return hops_of(a, (b, _EMPTY, a), 8, levels, max_sync, shard_bits, shard)


@functools.lru_cache(maxsize=None)
def wide_hops(depth, levels, max_sync=None):
    """X = wide_pair()'s side B against its side A and itself."""
    a, b = P.wide_pair()
    return hops_of(b, (a, b), depth, levels, max_sync)


def bad_position(rc):
    """a node form whose last position is 2^level: outside the tree"""
    assert rc[0] == "node"
    pos = np.array(rc[2], np.uint64)
    pos[-1] = np.uint64(1) << np.uint64(rc[1])
    return ("node", rc[1], pos, rc[3])


def empty_input(level):
    return ("node", level, np.zeros(0, np.uint64), np.zeros(0, np.uint64))
