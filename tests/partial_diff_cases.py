"""Inputs for the partial Merkle diff (csrc/merkle_cont.hip) that hashed one-row-per-key
replicas never make, and one ping-pong driver that walks the device and the C oracle hop
for hop (helper module: no tests).

ladder(): a crafted pair over 2^depth buckets whose bucket sizes step across the kernel's
register limits (BR = 16 rows, loaded in two rounds of 8), with keys that own one row,
every row or runs of three rows, and with every one-sided edit: a key only A holds, a key
only B holds (below every key, at the bucket's last possible key), a bucket empty on one
side.  wide_pair(): multi-row keys and different key sets, more differing buckets than the
home path's one-bucket-per-thread limit.  Test data only (seeded numpy)."""
import functools

import numpy as np

from delta_crdt_ex_amd import workloads as W
from oracle import ref as R

SIZES = [0, 1, 2, 7, 8, 9, 15, 16, 17, 18, 33]  # rows of A's bucket, around 8 | 16 | 17
PATTERNS, EDITS = 3, 6
N_CLASSES = len(SIZES) * PATTERNS * EDITS  # 198: buckets 1..198
STEP = 16                                  # key offsets 16, 32, ... inside a bucket
HOME_ENTRIES, HOME_BUCKETS = 4096, 512     # dg_merkle_continue_home's limits (CS_IN, CS_B)


def _bucket_keys(size, pattern):
    """Key offsets (from the bucket's first key) of a bucket's `size` rows."""
    i = np.arange(size, dtype=np.uint64)
    if pattern == 0:    # every row its own key
        return (i + np.uint64(1)) * np.uint64(STEP)
    if pattern == 1:    # one key owns every row
        return np.full(size, STEP, np.uint64)
    return (i // np.uint64(3) + np.uint64(1)) * np.uint64(STEP)  # runs of three: 7|8 and 15|16 straddled


@functools.lru_cache(maxsize=None)
def ladder(depth=8, shard_bits=0, shard=0):
    """(rows_a, rows_b, classes).  Bucket b of 1..198 is class c = b - 1: SIZES[c % 11]
    rows in A, key pattern (c // 11) % 3, B's edit (c // 33) % 6:
      0 identical            1 ts + 1 on the bucket's last row     2 B lacks the first key
      3 B adds offset 1      4 B adds the bucket's last key        5 B's bucket is empty
    Buckets 0 and 199.. hold three single-row keys, identical on both sides, except that
    bucket 0's first key sits at offset 0 and only A holds it, and the last bucket gets
    edit 4 (2^64 - 1, or the shard's last key, only in B).  classes: (size, pattern, edit)
    -> bucket, and ("spare", "first") / ("spare", "last")."""
    assert depth >= 8 and shard < (1 << shard_bits)
    rng = np.random.default_rng(1000 + 16 * shard_bits + shard)
    shift = 64 - shard_bits - depth
    base = (shard << (64 - shard_bits)) if shard_bits else 0
    nbk = 1 << depth
    a_keys, b_add, b_drop_bucket, b_drop_key, b_bump = [], [], [], [], []
    classes = {}
    n_rows = 0
    for b in range(nbk):
        first = base + (b << shift)
        last_key = first + (1 << shift) - 1
        if 1 <= b <= N_CLASSES:
            c = b - 1
            size, pattern, edit = SIZES[c % 11], (c // 11) % PATTERNS, (c // 33) % EDITS
            classes[(size, pattern, edit)] = b
            offs = _bucket_keys(size, pattern)
        else:
            size, pattern, edit = 3, 0, 0
            offs = _bucket_keys(3, 0)
            if b == 0:
                offs = offs.copy()
                offs[0] = 0
                edit = 2  # the first key (offset 0) is A-only
                classes[("spare", "first")] = b
            elif b == nbk - 1:
                edit = 4
                classes[("spare", "last")] = b
        keys = np.uint64(first) + offs
        a_keys.append(keys)
        n_rows += size
        if edit == 1 and size:
            b_bump.append(n_rows - 1)  # A's row index of the bucket's last row
        elif edit == 2 and size:
            b_drop_key.append(int(keys[0]))
        elif edit == 3:
            b_add.append(first + 1)
        elif edit == 4:
            b_add.append(last_key)
        elif edit == 5:
            b_drop_bucket.append(b)
    key = np.concatenate(a_keys)
    n = len(key)
    val = np.uint64(1 << 62) + rng.integers(0, 1 << 20, n).astype(np.uint64)
    ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    node = rng.integers(0, 4, n).astype(np.uint32)
    cnt = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    # B: A's rows edited
    keep = np.ones(n, bool)
    keep &= ~np.isin(key, np.array(b_drop_key, np.uint64))
    bucket = ((key - np.uint64(base)) >> np.uint64(shift)).astype(np.int64)
    keep &= ~np.isin(bucket, np.array(b_drop_bucket, np.int64))
    ts_b = ts.copy()
    ts_b[np.array(b_bump, np.int64)] += 1
    m = len(b_add)
    add = (np.array(b_add, np.uint64), np.uint64(1 << 62) + rng.integers(0, 1 << 20, m).astype(np.uint64),
           rng.integers(-(1 << 40), 1 << 40, m).astype(np.int64), rng.integers(0, 4, m).astype(np.uint32),
           np.arange(n + 1, n + m + 1, dtype=np.uint64))
    rows_a = W.sort_rows(key, val, ts, node, cnt)
    rows_b = W.sort_rows(*(np.concatenate([x[keep], y]) for x, y in zip((key, val, ts_b, node, cnt), add)))
    for r in rows_a + rows_b:
        r.setflags(write=False)
    return rows_a, rows_b, classes


def empty_rows():
    return (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint32),
            np.zeros(0, np.uint64))


@functools.lru_cache(maxsize=None)
def wide_pair():
    """Multi-row keys, different key sets: 1448 of 2048 buckets differ at depth 11, 1900
    of 4096 at depth 12 (both over the home path's 512 one-thread buckets)."""
    a, b = W.random_pair(np.random.default_rng(7), 3000, n_nodes=4, max_entries=3)
    return a["rows"], b["rows"]


def over_home_limits(rc):
    """Does this (oracle) continuation exceed what dg_merkle_continue_home takes?"""
    if rc[0] == "leaf":
        return len(rc[2]) > HOME_ENTRIES or len(rc[1]) > HOME_BUCKETS
    return len(rc[2]) > HOME_ENTRIES


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def assert_cont_equals(cont, rc, depth):
    """A device continuation (store.MerkleCont) against the oracle's tuple, every field."""
    if rc[0] == "node":
        assert cont.level == rc[1] and not cont.leaf and cont.n_buckets == 0
    else:
        assert cont.level == depth + 1
        assert cont.n_buckets == len(rc[1])
        assert np.array_equal(_u64(cont.bucket[: cont.n_buckets]), rc[1])
    assert cont.n == len(rc[2])
    assert np.array_equal(_u64(cont.pos[: cont.n]), rc[2])
    assert np.array_equal(_u64(cont.hash[: cont.n]), rc[3])


def run_protocol(first, second, levels, max_sync=None, mode="general", engine=None):
    """prepare_partial_diff on `first`, then continue_partial_diff ping-pong starting on
    `second`, each {:continue, c} truncated to max_sync (None: :infinite) before it is sent.
    first / second: (device tree or None, oracle tree, rows).  With an engine the device
    walks beside the oracle and every hop is compared with it: status, level, positions or
    keys, hashes, buckets and the counts.  mode "general": merkle_continue (+ merkle_truncate);
    "home": merkle_continue_home, the general calls only where it declines -- which must be
    exactly the hops whose input is over its limits.
    Returns a dict: keys (the oracle's; the device's are asserted equal), hops, sizes (per
    continuation sent: (n, n_buckets)), homed, kept (the buckets of the last leaf form sent,
    None if none was) and conts (the oracle's continuations, the prepared one first)."""
    assert mode in ("general", "home")
    depth = first[1].depth
    rc = R.merkle_prepare(first[1], levels)
    cont = None
    if engine is not None:
        cont = engine.merkle_prepare(first[0], levels)
        assert_cont_equals(cont, rc, depth)
    side = [second, first]
    hops = homed = 0
    sizes, conts, kept = [], [rc], None
    while True:
        t, r, rows = side[hops % 2]
        rres = R.merkle_continue(r, rows, rc, levels)
        if rres[0] == "continue" and max_sync is not None:
            rres = ("continue", R.merkle_truncate(r, rres[1], max_sync))
        if engine is not None:
            res = ("declined",)
            if mode == "home":
                res = engine.merkle_continue_home(t, cont, levels, max_sync)
                assert (res[0] == "declined") == over_home_limits(rc), (hops, rc[0], len(rc[2]))
                homed += res[0] != "declined"
            if res[0] == "declined":
                res = engine.merkle_continue(t, cont, levels)
                if res[0] == "continue" and max_sync is not None:
                    engine.merkle_truncate(t, res[1], max_sync)
            assert res[0] == rres[0], (hops, res[0], rres[0])
        hops += 1
        assert hops <= 2 * depth + 4, "the protocol does not end"
        if rres[0] == "ok":
            if engine is not None:
                assert res[2] == len(rres[1])
                assert np.array_equal(_u64(res[1]), rres[1])
            break
        rc = rres[1]
        conts.append(rc)
        if rc[0] == "leaf":
            kept = rc[1]
        sizes.append((len(rc[2]), len(rc[1]) if rc[0] == "leaf" else 0))
        if engine is not None:
            cont = res[1]
            assert_cont_equals(cont, rc, depth)
    return {"keys": rres[1], "hops": hops, "sizes": sizes, "homed": homed, "kept": kept, "conts": conts}


def kept_keys(full, tree, kept):
    """The differing keys a truncated protocol run ends in: those of the buckets the last
    leaf form kept (none when a truncated node form ended it in {:ok, []})."""
    if kept is None:
        return full[:0]
    return full[np.isin(tree.bucket_of(full), np.asarray(kept).astype(np.int64))]
