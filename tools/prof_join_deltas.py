"""dg_join_deltas against its parts and against k sequential dg_join_delta_diffs.

States: a config-3 shard (10M keys) and a config-4-sized state (12.5M keys), both built by the
config-3 generator; batches of k in {2, 8, 64} sync deltas of 200 keys and of ~1 % of the keys
each.  Per shape the variants alternate in one process, each call timed with device events on
its engine's stream, the state (rows, context, tree) restored from a pristine device copy
outside every timed window; at least 5 rounds, min - max over the rounds:

    fold      dg_apply_deltas alone (into the spare store)
    sdiff     dg_store_diff alone (the state against the folded result, with diffs)
    batch/r   dg_join_deltas with tree and diffs, the tree rebuilt   (DG_TREE_REBUILD=always)
    batch/u   dg_join_deltas with tree and diffs, the tree updated   (DG_TREE_REBUILD=never)
    seq       k sequential dg_join_delta_diffs
    keyed     dg_join_deltas_keyed with tree and diffs (a thread per key of the keysets' union);
              before timing its state, context, tree and changed keys are compared with batch/u's

    python tools/prof_join_deltas.py                  # the table (--small: 1M / 1.25M keys;
                                                      # --k 2,3,4,8,64: the batch sizes; --states 1:
                                                      # the config-4-sized state alone)
    python tools/prof_join_deltas.py --trace 5        # 5 dg_join_deltas calls per tree mode on the
                                                      # config-3 shard, k = 64 x 1 %: the target of a
                                                      # kernel-trace run of its own
    python tools/prof_join_deltas.py --trace-keyed 5  # 5 dg_join_deltas_keyed calls on the config-4-sized
                                                      # state (12.5M keys; with --small 1.25M, as DESIGN 4.17's
                                                      # split), k = 64 x 200 keys: the same for the keyed call
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delta_crdt_ex_amd import workloads as W  # noqa: E402
from delta_crdt_ex_amd.store import Context, Engine, Store  # noqa: E402

DEV = "cuda:0"
COLS = ("key", "val", "ts", "node", "cnt")
DEPTH = 20


def engine(tree_mode):
    os.environ["DG_TREE_REBUILD"] = tree_mode
    try:
        return Engine(0)
    finally:
        del os.environ["DG_TREE_REBUILD"]


def timed(eng, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def keys_dev(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(DEV)


class Shape:
    """One state and one batch on the device, with the pristine copies the state is restored from."""

    def __init__(self, eng, base, deltas):
        self.ds = [Store.from_numpy(*d["rows"], device=DEV) for d in deltas]
        self.dcs = [Context.from_numpy(d["ctx"][0], d["ctx"][1], d["ctx"][2], DEV) for d in deltas]
        self.ks = [keys_dev(d["keys"]) for d in deltas]
        n = len(base["rows"][0])
        self.total = n + sum(d.n for d in self.ds)
        self.ctx_total = len(base["ctx"][1]) + sum(c.n for c in self.dcs)
        self.pr_rows = Store.from_numpy(*base["rows"], device=DEV)
        self.pr_ctx = Context.from_numpy(base["ctx"][0], base["ctx"][1], base["ctx"][2], DEV)
        self.st, self.spare, self.out = (Store.empty(self.total, DEV) for _ in range(3))
        self.ctx = Context.empty(0, self.ctx_total, DEV)
        self.out_ctx = Context.empty(0, self.ctx_total, DEV)
        self.pr_tree = eng.merkle_build(self.pr_rows, DEPTH)
        self.tree = self.pr_tree.clone()
        self.changed = torch.empty(sum(int(k.numel()) for k in self.ks) + 64, dtype=torch.int64, device=DEV)
        self.restore()
        # the folded result, for the diff alone
        self.joined, _ = eng.apply_deltas(self.st, self.ctx, self.ds, self.dcs, self.ks,
                                          out=Store.empty(self.total, DEV), out_ctx=Context.empty(0, self.ctx_total, DEV))

    def restore(self):
        n = self.pr_rows.n
        for f in COLS:
            getattr(self.st, f)[:n].copy_(getattr(self.pr_rows, f)[:n])
        self.st.n = n
        m = self.pr_ctx.n
        self.ctx.node[:m].copy_(self.pr_ctx.node[:m])
        self.ctx.cnt[:m].copy_(self.pr_ctx.cnt[:m])
        self.ctx.n, self.ctx.kind = m, self.pr_ctx.kind
        self.tree.nodes.copy_(self.pr_tree.nodes)
        self.tree.counts.copy_(self.pr_tree.counts)
        self.tree.starts.copy_(self.pr_tree.starts)
        self.tree.n_keys = self.pr_tree.n_keys
        self.tree.store = self.st
        torch.cuda.synchronize()


def variants(sh, eng_r, eng_u):
    def fold():
        eng_r.apply_deltas(sh.st, sh.ctx, sh.ds, sh.dcs, sh.ks, out=sh.out, out_ctx=sh.out_ctx)

    def sdiff():
        eng_r.store_diff(sh.st, sh.joined, want_diffs=True, changed=sh.changed)

    def batch(eng):
        return lambda: eng.join_deltas(sh.st, sh.ctx, sh.ds, sh.dcs, sh.ks, sh.spare, sh.tree, changed=sh.changed)

    def seq():
        for d, c, k in zip(sh.ds, sh.dcs, sh.ks):
            eng_r.join_delta_diffs(sh.st, sh.ctx, d, c, k, sh.spare, sh.tree, changed=sh.changed)

    def keyed():
        got = eng_u.join_deltas_keyed(sh.st, sh.ctx, sh.ds, sh.dcs, sh.ks, sh.spare, sh.tree, changed=sh.changed)
        assert got is not None, "dg_join_deltas_keyed declined the batch"
        return got

    return [("fold", eng_r, fold), ("sdiff", eng_r, sdiff), ("batch/r", eng_r, batch(eng_r)),
            ("batch/u", eng_u, batch(eng_u)), ("seq", eng_r, seq), ("keyed", eng_u, keyed)]


def same_results(sh, a, b):
    """variants a and b leave the same state, context, tree and changed keys (and say whether
    the keyed call moved rows)"""
    got = []
    for fn in (a, b):
        sh.restore()
        ch, ov, nv, fl, sw = fn()
        torch.cuda.synchronize()
        n = sh.st.n
        got.append(([getattr(sh.st, f)[:n].clone() for f in COLS], sh.ctx.node[:sh.ctx.n].clone(),
                    sh.ctx.cnt[:sh.ctx.n].clone(), sh.tree.nodes.clone(), sh.tree.counts.clone(), sh.tree.n_keys,
                    ch.clone(), ov.clone(), nv.clone(), fl.clone()))
    x, y = got
    assert all(torch.equal(p, q) for p, q in zip(x[0], y[0])) and x[5] == y[5]
    assert all(torch.equal(p, q) for p, q in zip(x[1:5] + x[6:], y[1:5] + y[6:]))
    return sw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--trace-keyed", type=int, default=0)
    ap.add_argument("--k", default="2,8,64")
    ap.add_argument("--states", default="0,1", help="which of the two states: 0 the config-3 shard, 1 the config-4-sized")
    a = ap.parse_args()
    eng_r, eng_u = engine("always"), engine("never")
    print("build digest", eng_r.lib.dg_build_digest().decode(), "device", torch.cuda.get_device_name(0))
    sizes = [("config-3 shard", 1_000_000 if a.small else 10_000_000),
             ("config-4-sized state", 1_250_000 if a.small else 12_500_000)]
    if a.trace:
        n = sizes[0][1]
        base, deltas = W.config3(n_keys=n, n_replicas=64, touch=0.01)
        sh = Shape(eng_r, base, deltas)
        for name, eng in (("rebuild", eng_r), ("update", eng_u)):
            for _ in range(a.trace):
                sh.restore()
                ch, *_ = eng.join_deltas(sh.st, sh.ctx, sh.ds, sh.dcs, sh.ks, sh.spare, sh.tree, changed=sh.changed)
            print(f"{a.trace} dg_join_deltas calls, tree {name}: {ch.numel()} changed keys of {n}")
        return
    if a.trace_keyed:  # (the config-4-sized state, 64 x 200 keys: the target of a kernel-trace run of its own)
        n = sizes[1][1]
        base, deltas = W.config3(n_keys=n, n_replicas=64, touch=200 / n)
        sh = Shape(eng_u, base, deltas)
        for _ in range(a.trace_keyed):
            sh.restore()
            ch, *_ = eng_u.join_deltas_keyed(sh.st, sh.ctx, sh.ds, sh.dcs, sh.ks, sh.spare, sh.tree, changed=sh.changed)
        print(f"{a.trace_keyed} dg_join_deltas_keyed calls: {ch.numel()} changed keys of {n}")
        return
    rounds = max(a.rounds, 5)
    for sname, n in (sizes[int(i)] for i in a.states.split(",")):
        for touch, tname in ((200 / n, "200 keys"), (0.01, "1 % of the keys")):
            base, all_deltas = W.config3(n_keys=n, n_replicas=64, touch=touch)
            for k in (int(x) for x in a.k.split(",")):
                sh = Shape(eng_r, base, all_deltas[:k])
                vs = variants(sh, eng_r, eng_u)
                moved = same_results(sh, vs[3][2], vs[5][2])
                t = {name: [] for name, _, _ in vs}
                n_changed = 0
                for r in range(rounds + 1):  # (round 0 warms the scratch buffers up)
                    for name, eng, fn in vs:
                        sh.restore()
                        us = timed(eng, fn)
                        if r:
                            t[name].append(us)
                    n_changed = int(eng_r.store_diff(sh.pr_rows, sh.joined, changed=sh.changed).numel())
                print(f"== {sname} ({n} keys), k = {k} deltas of {tname}: {n_changed} keys changed, "
                      f"{rounds} rounds, us min - max (median)")
                for name, _, _ in vs:
                    v = np.array(t[name])
                    print(f"   {name:8s} {v.min():10.1f} - {v.max():10.1f}  ({np.median(v):10.1f})")
                f, b = np.median(t["fold"]), min(np.median(t["batch/r"]), np.median(t["batch/u"]))
                print(f"   post-pass over the plain fold: {b - f:.1f} us; batch / seq = {b / np.median(t['seq']):.3f}")
                print(f"   keyed == batch/u byte for byte; rows {'moved through the spare store' if moved else 'joined in place'}")
                del sh
                torch.cuda.empty_cache()
    eng_r.close()
    eng_u.close()


if __name__ == "__main__":
    main()
