"""The config-4 anti-entropy round's first two calls against the one that replaces them, on the
config-4 shard (12.5M keys, 1 % differing, the depth bench.py picks): alternating, as synchronous
C-ABI calls with arguments built beforehand,
  (a) dg_merkle_diff followed by dg_take_keys   -- code the take form does not touch: the baseline
  (b) dg_merkle_diff_take
and prints both medians and (a)'s max - min spread.  (b) is faster when its median is below (a)'s
by more than that spread.

    python tools/prof_diff_take.py [--reps 9] [--leg a|b]    # --leg: one leg only, for a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delta_crdt_ex_amd import _abi  # noqa: E402
from delta_crdt_ex_amd import workloads as W  # noqa: E402
from delta_crdt_ex_amd.store import Engine, MerkleTree, Store, TermHashes, u64  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--keys", type=int, default=12_500_000)
ap.add_argument("--leg", choices=["a", "b", "both"], default="both")
ap.add_argument("--sync", type=int, default=0, metavar="N",
                help="also time dgr_sync_from (src = B toward dst = A, every differing key) N times through "
                     "the replica layer, each on a freshly loaded dst: reported beside the round's three calls")
args = ap.parse_args()
assert args.reps >= 7

a, b = W.config4_shard(0, 1, keys_per_rank=args.keys, diff_frac=0.01)
dev = "cuda:0"
eng = Engine(0)
terms = TermHashes(*a["nodes"].universe.term_tables(), dev)
sa, sb = Store.from_numpy(*a["rows"], device=dev), Store.from_numpy(*b["rows"], device=dev)
depth = max(8, min(28, int(np.ceil(np.log2(max(args.keys, 2) / 3)))))  # bench.py's choice
ta = eng.merkle_build(sa, depth, MerkleTree.empty(depth, dev, 0, 0, terms), 0, 0)
tb = eng.merkle_build(sb, depth, MerkleTree.empty(depth, dev, 0, 0, terms), 0, 0)

# sizes from one untimed round through the binding; then every argument is built once
keys, rows, offs, total = eng.merkle_diff_take(ta, tb, side=1)
ref_keys = eng.merkle_diff(ta, tb)
ref_rows = eng.take_keys(sb, ref_keys)
assert total == keys.numel() and torch.equal(keys, ref_keys) and rows.n == ref_rows.n
for g, e in zip(rows.to_numpy(), ref_rows.to_numpy()):
    assert np.array_equal(g, e)
cap = total + 1024
out_a = torch.empty(cap, dtype=torch.int64, device=dev)
out_b = torch.empty(cap, dtype=torch.int64, device=dev)
offs_b = torch.empty(cap + 1, dtype=torch.int64, device=dev)
rows_a, rows_b = Store.empty(rows.n + 1024, dev), Store.empty(rows.n + 1024, dev)
tas, tbs, sas, sbs = ta.abi(), tb.abi(), sa.abi(), sb.abi()
ra, rb = rows_a.abi(), rows_b.abi()
n, tot = C.c_uint64(), C.c_uint64()
P = lambda t: C.cast(t.data_ptr(), _abi.P64)
refs = [C.byref(x) for x in (tas, sas, tbs, sbs)]
pa, pb, po = P(out_a), P(out_b), P(offs_b)
lib, h = eng.lib, eng.h


def leg_a():
    rc = lib.dg_merkle_diff(h, refs[0], refs[1], refs[2], refs[3], pa, cap, C.byref(n), C.byref(tot))
    rc |= lib.dg_take_keys(h, refs[3], pa, n.value, C.byref(ra))
    return rc


def leg_b():
    return lib.dg_merkle_diff_take(h, refs[0], refs[1], refs[2], refs[3], 1, pb, cap, po, C.byref(rb), C.byref(n),
                                   C.byref(tot))


legs = {"a": leg_a, "b": leg_b}
if args.leg != "both":
    legs = {args.leg: legs[args.leg]}
res = {k: [] for k in legs}
torch.cuda.synchronize()
for rep in range(args.reps + 2):
    for name, f in legs.items():
        t0 = time.perf_counter()
        rc = f()
        dt = time.perf_counter() - t0
        assert rc == 0, lib.dg_last_error()
        if rep >= 2:
            res[name].append(dt * 1e6)
summary = {"keys": args.keys, "depth": depth, "differing": total, "rows": rows.n, "reps": args.reps}
for k, v in res.items():
    summary[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                  "spread_us": round(max(v) - min(v), 1), "all_us": [round(x, 1) for x in v]}
if len(res) == 2:
    summary["b_faster_by_us"] = round(summary["a"]["median_us"] - summary["b"]["median_us"], 1)
    summary["done"] = summary["b_faster_by_us"] > summary["a"]["spread_us"]
if args.sync:
    # the replica layer on an engine of its own: both replicas resident, trees of the same depth
    from delta_crdt_ex_amd import nif  # noqa: E402
    rl = nif.load()
    g = C.c_void_p()
    assert rl.dgr_engine_open(0, C.byref(g)) == 0
    nh, vid, vh = a["nodes"].universe.term_tables()
    assert rl.dgr_refresh_terms(g, nh.ctypes.data, len(nh), vid.ctypes.data, vh.ctypes.data, len(vid)) == 0

    def load(rep):
        cols = [np.ascontiguousarray(c, dt)
                for c, dt in zip(rep["rows"], (np.uint64, np.uint64, np.int64, np.uint32, np.uint64))]
        kind, cn, cc = rep["ctx"]
        cn, cc = np.ascontiguousarray(cn, np.uint32), np.ascontiguousarray(cc, np.uint64)
        st = _abi.dg_store(*(c.ctypes.data for c in cols), len(cols[0]), len(cols[0]))
        cx = _abi.dg_context(kind=int(kind), node=cn.ctypes.data, cnt=cc.ctypes.data, n=len(cn), cap=len(cn))
        p = C.c_void_p()
        assert rl.dgr_state_load(g, C.byref(st), C.byref(cx), C.byref(p)) == 0
        assert rl.dgr_merkle_build(p, 1, depth) == 0
        return p

    src = load(b)
    times = []
    for rep in range(args.sync):
        dst = load(a)
        ch, n_tot = nif.dgr_changed(), C.c_uint64()
        t0 = time.perf_counter()
        rc = rl.dgr_sync_from(dst, 1, src, 1, 0, C.byref(ch), C.byref(n_tot))
        dt = time.perf_counter() - t0
        assert rc == 0 and n_tot.value == total, (rc, n_tot.value, lib.dg_last_error())
        times.append(round(dt * 1e6, 1))
        summary["sync_changed"] = int(ch.n_changed)
        assert rl.dgr_state_free(dst) == 0
    summary["sync_from_us"] = {"median_us": float(np.median(times)), "all_us": times,
                               "note": "the first call also grows the engine's buffers"}
    assert rl.dgr_state_free(src) == 0 and rl.dgr_engine_close(g) == 0
print(json.dumps(summary))
