"""Inputs that drive the take hop (csrc/merkle_cont.hip take_hop, cont_hop_kernel<true, true>)
past one staging pass of CS_IN = 4096 output rows and to the 2^22 rows at which its block scan
changes form (helper module: no tests, no GPU; seeded numpy, read-only arrays).

stairs(): a replica X of 16,440 rows in the 512 buckets of a depth-9 tree and a peer P = X edited.
Bucket b of X holds
  b == LONG_BUCKET : one key of 8200 rows, alone (more than two passes; no longer, so that the
                     other 511 buckets hold 8240 rows: a take of exactly 8192 rows cannot hold
                     this key, and all of X has to stay within the replica layer's room);
  b % 4 == 3       : 17 .. 40 rows ("big": the kernel walks global memory), single-row keys and
                     runs of three in turn;
  else             : at most 16 rows ("reg": the kernel's register path), keys of 1, 3 or 5 rows
                     and then single-row keys up to the 16,440 rows in all;
so both kinds lie on both sides of the rows 4096, 8192 and 12288, and more than 4096 rows lie
before the long key.  P's edit of bucket b is (b // 4) % 6, independent of the bucket's kind:
  0 ts + 1 on the last row of the bucket's last key (the keys before it identical)
  1 P lacks the bucket's second key (the first identical)
  2 P adds a key between the first and the second key and the bucket's last possible key, and
    the last key's last row is bumped
  3 P's bucket is empty
  4 the last row of every key but the first is bumped
  5 identical
except that buckets 0 .. 7 are identical (so every row P's leaf forms take has a store index
above its output index) and the long key has its last row bumped.  P holds fewer than 4096
distinct keys: no leaf form X receives is over the home path's limits.

hops(max_sync): what X answers -- its conversations with P and with an empty replica (whose
last hop takes all of X: 16,440 rows, five passes, inside the replica layer's room of
min(rows, 4 * 4096 + 64) = 16,440 rows) and the crafted leaf forms of CRAFTED, each with the C
oracle's answer.  A crafted form lists the buckets [s, e) but those left out, with no pairs
("all": every key of the buckets differs), with P's pairs ("p"), or with P's pairs of the keys X
lacks ("only": every key of X differs and those keys come between them, without rows).  The
ranges were found by a search over such ranges for the situations key_paths() names; the CPU
test tests/test_take_pass_cases.py proves that they, with CUTS, reach every one.

huge(): 2^22 + 1 rows at depth 9, for the scan's totals 2^22 - 1, 2^22 and 2^22 + 1."""
import functools

import numpy as np

import cont_batch_cases as B
import partial_diff_cases as P
from delta_crdt_ex_amd import workloads as W
from oracle import ref as R

DEPTH, LEVELS = 9, 3
NBK, SHIFT = 1 << DEPTH, 64 - DEPTH
PASS = 4096            # CS_IN: output rows staged per pass
BR = 16                # rows of a bucket the hop kernel keeps in registers
LONG_BUCKET, LONG_ROWS = 300, 8200
X_ROWS = 16440         # within (16384, 16448]: the take of all of X is five passes and fits the room
STEP = 16              # key offsets 16, 32, ... inside a bucket
ROOM_KEYS, ROOM_EXTRA = 4096, 64  # replica_pack.h rp_take_room_for: R = min(rows_n, 4 * min(kcap, 4096) + 64)

# (mode, first bucket, end bucket, buckets left out)
CRAFTED = (("all", 1, 512, (7, 300)),      # 8192 rows
           ("only", 0, 512, (75,)),        # 16,414 rows, a key X lacks at row 4096 p
           ("all", 45, 301, (155, 300)),   # 4097 rows
           ("all", 45, 301, (67, 300)),    # 4096 rows
           ("all", 64, 512, ()))           # four passes
# the max_sync values (besides None) the cases run: at 2247 a cut falls inside a register bucket
# in one hop and inside a big one in another, both past row 4096 and before the long key
CUTS = (2247,)
CASES = (None,) + CUTS  # the max_sync of every parity case: hops(m) for m in CASES is what the GPU files run

SITUATIONS = frozenset({
    "reg_straddle", "big_straddle", "reg_ends_at", "big_ends_at", "absent_at", "whole_pass", "total_4096",
    "total_4097", "total_8192", "cut_reg_late", "cut_big_late", "skipped_late", "shifted", "five_passes"})


def _x_buckets(rng):
    """per bucket the row counts of its keys"""
    out = []
    for b in range(NBK):
        if b == LONG_BUCKET:
            out.append([LONG_ROWS])
        elif b % 4 == 3:
            size, keys = int(rng.integers(BR + 1, 41)), []
            while sum(keys) < size:
                keys.append(min(3 if len(keys) % 2 else 1, size - sum(keys)))
            out.append(keys)
        else:
            keys = [int(x) for x in rng.choice([1, 3, 5], int(rng.integers(2, 6)))]
            while sum(keys) > BR:
                keys.pop()
            out.append(keys)
    # to X_ROWS exactly: single-row keys added to / last keys dropped from register buckets in turn
    reg = [b for b in range(NBK) if b != LONG_BUCKET and b % 4 != 3]
    i = 0
    while sum(map(sum, out)) != X_ROWS:
        keys = out[reg[i % len(reg)]]
        i += 1
        short = X_ROWS - sum(map(sum, out))
        if short > 0 and sum(keys) < BR:
            keys.append(1)
        elif short < 0 and len(keys) > 2 and keys[-1] <= -short:
            keys.pop()
    return out


@functools.lru_cache(maxsize=None)
def stairs():
    """(rows_x, rows_p)"""
    rng = np.random.default_rng(4096)
    per_bucket = _x_buckets(rng)
    step = np.uint64(STEP)
    key = np.concatenate([np.repeat(np.uint64(b << SHIFT) + step * np.arange(1, len(ks) + 1, dtype=np.uint64), ks)
                          for b, ks in enumerate(per_bucket)])
    n = len(key)
    assert n == X_ROWS
    val = np.uint64(1 << 62) + rng.integers(0, 1 << 20, n).astype(np.uint64)
    ts = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    node = rng.integers(0, 4, n).astype(np.uint32)
    cnt = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    rows_x = W.sort_rows(key, val, ts, node, cnt)
    # P: X's sorted rows edited
    xk = rows_x[0]
    keep = np.ones(n, bool)
    ts_p = rows_x[2].copy()
    add = []

    def last_row(k):
        return int(np.searchsorted(xk, np.uint64(k), "right")) - 1

    for b, ks in enumerate(per_bucket):
        first = b << SHIFT
        keys = [first + STEP * (i + 1) for i in range(len(ks))]
        edit = (b // 4) % 6
        if b == LONG_BUCKET:
            ts_p[last_row(keys[0])] += 1
        elif b < 8 or edit == 5:
            continue
        elif edit == 0:
            ts_p[last_row(keys[-1])] += 1
        elif edit == 1:
            keep &= xk != np.uint64(keys[1])
        elif edit == 2:
            add += [keys[0] + STEP // 2, first + (1 << SHIFT) - 1]
            ts_p[last_row(keys[-1])] += 1
        elif edit == 3:
            keep &= (xk >> np.uint64(SHIFT)) != np.uint64(b)
        else:
            for k in keys[1:]:
                ts_p[last_row(k)] += 1
    m = len(add)
    extra = (np.array(add, np.uint64), np.uint64(1 << 62) + rng.integers(0, 1 << 20, m).astype(np.uint64),
             rng.integers(-(1 << 40), 1 << 40, m).astype(np.int64), rng.integers(0, 4, m).astype(np.uint32),
             np.arange(n + 1, n + m + 1, dtype=np.uint64))
    rows_p = W.sort_rows(*(np.concatenate([x[keep], y])
                           for x, y in zip((xk, rows_x[1], ts_p, rows_x[3], rows_x[4]), extra)))
    for r in rows_x + rows_p:
        r.setflags(write=False)
    return rows_x, rows_p


def crafted_buckets(s, e, dropped):
    b = np.arange(s, e, dtype=np.uint64)
    return b[~np.isin(b, np.array(dropped, np.uint64))]


@functools.lru_cache(maxsize=None)
def crafted_conts():
    """the crafted leaf forms X receives, in CRAFTED's order"""
    rows_x, rows_p = stairs()
    tp = B.tree_of(rows_p, DEPTH)
    out = []
    for mode, s, e, dropped in CRAFTED:
        buckets = crafted_buckets(s, e, dropped)
        pk, ph = R.leaf_pairs(rows_p, tp, buckets) if mode != "all" else (np.zeros(0, np.uint64),) * 2
        if mode == "only":
            lacks = ~np.isin(pk, rows_x[0])
            pk, ph = pk[lacks], ph[lacks]
        out.append(("leaf", buckets, pk, ph))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hops_of_conversations(max_sync=None):
    """(cont, want) of every hop X answers in its conversations with P and the empty replica"""
    rows_x, rows_p = stairs()
    return tuple(B.hops_of(rows_x, (rows_p, P.empty_rows()), DEPTH, LEVELS, max_sync))


@functools.lru_cache(maxsize=None)
def hops(max_sync=None):
    """hops_of_conversations, then the crafted leaf forms"""
    rows_x, _ = stairs()
    tx = B.tree_of(rows_x, DEPTH)
    return hops_of_conversations(max_sync) + tuple(
        (rc, B.answer(tx, rows_x, rc, LEVELS, max_sync)) for rc in crafted_conts())


def replica_room(rows_n, n_in, max_sync):
    """the rows the replica layer gives a leaf form of n_in pairs for its take (replica_pack.h):
    rp_take_room_for's R = min(rows_n, 4 * min(kcap, 4096) + 64) with rp_cont_room_for's
    kcap = max(min(max_sync, rows_n + n + 1, 65536), 1)"""
    kcap = max(min(rows_n + n_in + 1, 65536, *([] if max_sync is None else [max_sync])), 1)
    return min(rows_n, 4 * min(kcap, ROOM_KEYS) + ROOM_EXTRA)


def kept_of(want, max_sync):
    """the keys a keys hop keeps: truncate(keys, max_sync_size)"""
    return want[1] if max_sync is None else want[1][:max_sync]


def row_total(rows_x, kept):
    return int(np.isin(rows_x[0], kept).sum())


def key_paths(rows_x, counts, keys, max_sync):
    """The situations of one keys answer (the oracle's `keys`, truncated to max_sync) in the pass
    loop, from numpy alone: n the kept keys' row counts in X, o their offsets in the output.
    counts: X's rows per bucket.  For a boundary B = 4096 p, p >= 1:
      reg_straddle / big_straddle : o < B < o + n, the key in a bucket of <= 16 / > 16 rows
      reg_ends_at / big_ends_at   : n > 0 and o + n == B
      absent_at                   : n == 0 and o == B, rows following
      whole_pass                  : o <= B and B + 4096 <= o + n
    total_4096 / total_4097 / total_8192 / five_passes (16384 < total <= 16448): the row total;
    cut_reg_late / cut_big_late: the last kept key and the first key cut share a bucket and the
    kept one's rows start at or past row 4096; skipped_late: a kept key with rows from row 4096 on,
    in a register bucket, whose predecessor in X lies in the same bucket and is not among the keys;
    shifted: more than one pass and no output row from 4096 on sits at its own store index."""
    xk = rows_x[0]
    keys = np.asarray(keys, np.uint64)
    kept = kept_of((None, keys), max_sync)
    lo, hi = np.searchsorted(xk, kept, "left"), np.searchsorted(xk, kept, "right")
    n = (hi - lo).astype(np.int64)
    o = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    total, o = int(o[-1]), o[:-1]
    bucket = (kept >> np.uint64(SHIFT)).astype(np.int64)
    big = np.asarray(counts)[bucket] > BR
    got = set()
    for bnd in range(PASS, total + 1, PASS):
        straddle = (o < bnd) & (bnd < o + n)
        ends = (n > 0) & (o + n == bnd)
        for name, m in (("straddle", straddle), ("ends_at", ends)):
            got |= {("big_" if g else "reg_") + name for g in set(big[m].tolist())}
        if np.any((n == 0) & (o == bnd)) and bnd < total:
            got.add("absent_at")
        if np.any((o <= bnd) & (bnd + PASS <= o + n)):
            got.add("whole_pass")
    got |= {"total_%d" % t for t in (4096, 4097, 8192) if total == t}
    if 4 * PASS < total <= 4 * ROOM_KEYS + ROOM_EXTRA:
        got.add("five_passes")
    if 0 < len(kept) < len(keys):
        nxt = int(keys[len(kept)] >> np.uint64(SHIFT))
        if nxt == bucket[-1] and n[-1] > 0 and o[-1] >= PASS:
            got.add("cut_big_late" if big[-1] else "cut_reg_late")
    ux = np.unique(xk)
    at = np.searchsorted(ux, kept)
    prev = ux[np.maximum(at - 1, 0)]
    skipped = ((n > 0) & (o >= PASS) & ~big & (at > 0) & ((prev >> np.uint64(SHIFT)).astype(np.int64) == bucket)
               & ~np.isin(prev, keys))
    if np.any(skipped):
        got.add("skipped_late")
    if total > PASS:
        src = np.repeat(lo - o, n) + np.arange(total)
        if np.all(src[PASS:] != np.arange(PASS, total)):
            got.add("shifted")
    return got


def pass_paths(rows_x, hops, max_sync):
    """the situations (key_paths) the keys hops among `hops` reach at this max_sync"""
    counts = B.tree_of(rows_x, DEPTH).counts
    got = set()
    for _, w in hops:
        if B.kind_of(w) == "keys":
            got |= key_paths(rows_x, counts, w[1], max_sync)
    return got


HUGE_LONG = 8191                      # rows of each bucket's first key
HUGE_ROWS = (1 << 22) + 1
HUGE_CUTS = (1023, 1024, None)        # max_sync: totals 2^22 - 1, 2^22, 2^22 + 1


@functools.lru_cache(maxsize=None)
def huge():
    """X of exactly 2^22 + 1 rows at depth 9: every bucket holds one key of 8191 rows and then a
    single-row key, and the LAST bucket a third key of one row -- 1025 keys.  (The third key has to
    follow every 8191-row key: the totals of the first 1023 and 1024 keys are 2^22 - 1 and 2^22
    only if the two keys cut last own one row each.)  Against a leaf form of all 512 buckets with
    no pairs every key differs: the keys expected are np.unique(key)[:max_sync], the row total
    their rows'.  Built sorted and passed through W.sort_rows; the oracle's Python row loops
    (leaf_pairs, merkle_continue) are never run on it."""
    first = np.arange(NBK, dtype=np.uint64) << np.uint64(SHIFT)
    key = np.concatenate([np.repeat(first + np.uint64(STEP), HUGE_LONG).reshape(NBK, HUGE_LONG),
                          (first + np.uint64(2 * STEP))[:, None]], 1).ravel()
    key = np.concatenate([key, first[-1:] + np.uint64(3 * STEP)])
    n = len(key)
    assert n == HUGE_ROWS
    i = np.arange(n, dtype=np.uint64)
    rows = W.sort_rows(key, np.uint64(1 << 62) + (i * np.uint64(2654435761)) % np.uint64(1 << 20),
                       (i.astype(np.int64) * 7919) % (1 << 41) - (1 << 40), (i % np.uint64(4)).astype(np.uint32),
                       i + np.uint64(1))
    for r in rows:
        r.setflags(write=False)
    return rows


def huge_expect(rows_x, max_sync):
    """(keys kept, total differing keys, rows of the kept keys) for the leaf form of all buckets
    with no pairs"""
    keys, per_key = np.unique(rows_x[0], return_counts=True)
    kept = keys if max_sync is None else keys[:max_sync]
    return kept, len(keys), int(per_key[: len(kept)].sum())


def huge_cont():
    return ("leaf", np.arange(NBK, dtype=np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
