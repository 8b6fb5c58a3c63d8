"""What dg_read_diff and dg_join_delta_diffs must give, from the C oracle: read/2
(ref.read_lww) of a key list on the rows before and after a join, as the three arrays of
dg_lww_diffs -- and the classes of changed keys the GPU tests require their inputs to hold."""
import numpy as np

from oracle import ref as R

OLD, NEW = 1, 2  # DG_DIFF_OLD, DG_DIFF_NEW


def _read(rows, keys):
    """(value ids, present) of read/2 for keys in the caller's order (repeats allowed)."""
    val, has = np.zeros(len(keys), np.uint64), np.zeros(len(keys), bool)
    if len(rows[0]) == 0 or len(keys) == 0:
        return val, has
    k, v = R.read_lww(rows, keys=keys)  # the present keys, ascending unique
    if len(k) == 0:
        return val, has
    pos = np.minimum(np.searchsorted(k, keys), len(k) - 1)
    has = k[pos] == keys
    val[has] = v[pos][has]
    return val, has


def expected_diffs(old_rows, new_rows, keys):
    """(old_val, new_val, flags) for `keys`: a value whose flag is clear is 0."""
    keys = np.asarray(keys, np.uint64)
    ov, oh = _read(old_rows, keys)
    nv, nh = _read(new_rows, keys)
    return ov, nv, (oh * OLD + nh * NEW).astype(np.uint8)


def classes(new_rows, keys, old_val, new_val, flags):
    """How many of `keys` read the same value before and after, are removed, are added, are
    updated, and have their new winner decided by the tie-break (several values at the
    maximal ts: the smallest wins)."""
    both = flags == OLD | NEW
    ties = 0
    k, v, t = new_rows[0], new_rows[1], new_rows[2]
    for key in np.asarray(keys, np.uint64)[(flags & NEW) != 0]:
        lo, hi = np.searchsorted(k, key, "left"), np.searchsorted(k, key, "right")
        top = t[lo:hi] == t[lo:hi].max()
        ties += len(np.unique(v[lo:hi][top])) > 1
    return {"unchanged": int((both & (old_val == new_val)).sum()), "removed": int((flags == OLD).sum()),
            "added": int((flags == NEW).sum()), "updated": int((both & (old_val != new_val)).sum()),
            "ties": int(ties)}
