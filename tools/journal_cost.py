"""What persisting a resident replica costs per delta, and what a restore costs.

A resident replica of --keys keys (default 1M) takes 200-key sync deltas.  Per delta: the time
and bytes of storage.write (the whole snapshot: all the parent commit could do) against
Journal.append of the delta's effect with fsync on and off.  Restore, for journals of 64 and
4,096 records: storage.read (base load + ONE dg_replace_keysets) against storage.read_arrays
(host replay_arrays) followed by the upload; and Engine.replace_keysets alone against ONE
dg_join_delta of the same key count, the yardstick for the splice the two share.  Medians with
the run-to-run spread (min..max over --reps runs, after one warm-up), host clock around calls
that end in a device wait.  Prints one JSON line; the digest names the library sources measured.

    python tools/journal_cost.py [--keys N] [--records 64,4096] [--reps R] [--dir D]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delta_crdt_ex_amd import _abi, storage  # noqa: E402
from delta_crdt_ex_amd import aw_lww_map as M  # noqa: E402
from delta_crdt_ex_amd import workloads as W  # noqa: E402
from delta_crdt_ex_amd.store import Context, Store, TermHashes, u64  # noqa: E402

DELTA_KEYS = 200


def stats(xs, unit=1e3):
    xs = [x * unit for x in xs]
    return {"median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "n": len(xs)}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kt(keys, dev):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64).copy()).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--records", default="64,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    eng = M.engine()
    dev = M._dev()
    A, B = W.merkle_pair(n_keys=a.keys, diff_frac=0.5)
    U = A["nodes"].universe
    depth = max(8, min(28, int(np.ceil(np.log2(a.keys / 3)))))
    differ = A["rows"][0][A["rows"][1] != B["rows"][1]]
    rng = np.random.default_rng(18)
    tmp = tempfile.mkdtemp(prefix="journal_cost_", dir=a.dir)
    out = {"keys": a.keys, "delta_keys": DELTA_KEYS, "tree_depth": depth, "sources": _abi.source_digest(),
           "device": torch.cuda.get_device_name(0)}

    def replica():
        """The base replica on the device: its context with room for a union, its tree, a spare."""
        kind, node, cnt = A["ctx"]
        ctx = Context.empty(kind, 64, dev)
        ctx.node[:len(node)].copy_(torch.from_numpy(node.view(np.int32).copy()))
        ctx.cnt[:len(node)].copy_(torch.from_numpy(cnt.view(np.int64).copy()))
        ctx.n = len(node)
        st = M.AWLWWMap(Store.from_numpy(*A["rows"], device=dev), ctx, U)
        tree = eng.merkle_build(st.rows, depth, terms=TermHashes.of(U, dev))
        return st, tree, Store.empty(a.keys + 4 * DELTA_KEYS + 4096, dev)

    N = A["nodes"]   # N[0] wrote the base, N[2] is the peer
    top = [a.keys]   # the peer's counter: every delta's dots are new to the replica

    def peer_delta(keys):
        """The peer's sync message for `keys` (ascending): its value and ts of each key under a
        fresh dot, and its context up to that dot (a peer that writes, then syncs)."""
        i = np.searchsorted(B["rows"][0], keys)
        n = len(keys)
        cnt = np.arange(top[0] + 1, top[0] + 1 + n, dtype=np.uint64)
        top[0] += n
        rows = (keys, B["rows"][1][i], B["rows"][2][i], np.full(n, N[2], np.uint32), cnt)
        return Store.from_numpy(*rows, device=dev), Context.from_numpy(*W.vv({N[0]: a.keys, N[2]: top[0]}), dev)

    def one_delta(st, tree, spare):
        """Join one 200-key sync delta; returns the record's parts (host arrays)."""
        keys = np.sort(rng.choice(differ, DELTA_KEYS, replace=False))
        delta, dctx = peer_delta(keys)
        rows = Store.empty(8 * DELTA_KEYS, dev)
        changed, *_ = eng.join_delta_diffs(st.rows, st.ctx, delta, dctx, kt(keys, dev), spare, tree, rows=rows)
        node, cnt = st.ctx.to_numpy()
        return u64(changed), rows.to_numpy(), (st.ctx.kind, node, cnt), tree.root()

    # ---- per delta
    st, tree, spare = replica()
    path = os.path.join(tmp, "per_delta.dgsnap")
    t_write, t_sync, t_nosync, b_rec = [], [], [], []
    j = storage.checkpoint(path, 1, 0, st, tree)
    for rep in range(a.reps + 1):
        parts = [one_delta(st, tree, spare) for _ in range(2)]
        ts, n1 = timed(lambda: j.append(j.sequence_number + 1, *parts[0], fsync=True))
        tn, n2 = timed(lambda: j.append(j.sequence_number + 1, *parts[1], fsync=False))
        if rep:
            t_sync.append(ts), t_nosync.append(tn), b_rec.extend([n1, n2])
    j.close()
    for rep in range(min(a.reps, 3) + 1):
        tw, _ = timed(lambda: storage.write(path, 1, rep, st, tree))
        if rep:
            t_write.append(tw)
    out["per_delta"] = {"write_ms": stats(t_write), "write_bytes": os.path.getsize(path),
                        "append_fsync_ms": stats(t_sync), "append_nofsync_ms": stats(t_nosync),
                        "record_bytes": stats(b_rec, 1)}

    # ---- restore
    out["restore"] = {}
    for n_rec in [int(x) for x in a.records.split(",")]:
        st, tree, spare = replica()
        path = os.path.join(tmp, f"restore_{n_rec}.dgsnap")
        j = storage.checkpoint(path, 1, 0, st, tree)
        for _ in range(n_rec):
            j.append(j.sequence_number + 1, *one_delta(st, tree, spare), fsync=False)
        j.close()
        live = st.rows.to_numpy()
        records = storage.read_journal(path)
        union = np.unique(np.concatenate([r["keys"] for r in records]))
        t_read, t_host, t_replace, t_join = [], [], [], []
        for rep in range(a.reps + 1):
            td, got = timed(lambda: storage.read(path))
            assert all(np.array_equal(x, y) for x, y in zip(got[2].rows.to_numpy(), live)) and got[3].root() == tree.root()
            del got

            def host():
                _, _, rows, ctx, _, _ = storage.read_arrays(path)
                return Store.from_numpy(*rows, device=dev), Context.from_numpy(ctx[0], ctx[1], ctx[2], dev)
            th, got = timed(host)
            assert got[0].n == len(live[0])
            del got
            # the one device call alone, on a fresh copy of the base, records already uploaded
            base, btree, _ = replica()
            key_off = np.concatenate([[0], np.cumsum([len(r["keys"]) for r in records])])
            row_off = np.concatenate([[0], np.cumsum([len(r["rows"][0]) for r in records])])
            kcat = kt(np.concatenate([r["keys"] for r in records]), dev)
            rcat = Store.from_numpy(*[np.concatenate([r["rows"][i] for r in records]) for i in range(5)],
                                    device=dev)
            bspare = Store.empty(base.rows.n + rcat.n, dev)
            tr, (_, r_swapped) = timed(lambda: eng.replace_keysets_cat(base.rows, kcat, key_off, rcat, row_off,
                                                                        bspare, btree))
            assert btree.root() == tree.root()
            # the yardstick: one keyed join of as many keys into the same base
            base, btree, _ = replica()
            delta, dctx = peer_delta(union)
            uk = kt(union, dev)
            bspare = Store.empty(base.rows.n + delta.n, dev)
            tj, (_, j_swapped) = timed(lambda: eng.join_delta(base.rows, base.ctx, delta, dctx, uk, bspare, btree))
            if rep:
                t_read.append(td), t_host.append(th), t_replace.append(tr), t_join.append(tj)
        out["restore"][str(n_rec)] = {
            "journal_bytes": os.path.getsize(storage.journal_path(path)), "union_keys": int(len(union)),
            "record_keys": int(sum(len(r["keys"]) for r in records)),
            "read_base_plus_replace_ms": stats(t_read), "host_replay_plus_upload_ms": stats(t_host),
            "replace_keysets_ms": stats(t_replace), "join_delta_same_keys_ms": stats(t_join),
            "replace_went_through_spare": bool(r_swapped), "join_went_through_spare": bool(j_swapped)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
