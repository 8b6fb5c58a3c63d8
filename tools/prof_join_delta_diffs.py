"""on_diffs from a resident state at the config-4 shape (a sync delta of the 1 % differing keys
into a 12.5M-key shard, with the tree): dg_join_delta_diffs against the three calls a caller
needs without it -- a keyed dg_read_lww of the keyset on the state, dg_join_delta_out, a
keyed dg_read_lww of the changed keys -- and against dg_join_delta_out alone (what the diffs
add to the call), in one process, alternating, the state restored between calls (untimed).
Host clock around synchronous calls; every output preallocated.  Under rocprofv3
--kernel-trace the same run gives kd_count_diffs_kernel beside kd_count_kernel.

    python tools/prof_join_delta_diffs.py [keys_per_rank] [reps]
"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delta_crdt_ex_amd import _abi  # noqa: E402
from delta_crdt_ex_amd import workloads as W  # noqa: E402
from delta_crdt_ex_amd.store import Context, Engine, MerkleTree, Store, TermHashes, u64  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
a, b = W.config4_shard(0, 8, keys_per_rank=n, diff_frac=0.01)
dev = "cuda:0"
eng = Engine(0)
lib = eng.lib
terms = TermHashes(*a["nodes"].universe.term_tables(), dev)
depth = int(np.ceil(np.log2(len(a["rows"][0]) / 3)))
sa = Store.from_numpy(*a["rows"], device=dev)
sb = Store.from_numpy(*b["rows"], device=dev)
ta = eng.merkle_build(sa, depth, MerkleTree.empty(depth, dev, 3, 0, terms), 3, 0)
tb = eng.merkle_build(sb, depth, MerkleTree.empty(depth, dev, 3, 0, terms), 3, 0)
keys = eng.merkle_diff(ta, tb)
nk = int(keys.numel())
d = W.sync_delta(b, keys.cpu().numpy().view(np.uint64))
sd = Store.from_numpy(*d["rows"], device=dev)
cd = Context.from_numpy(*d["ctx"], dev)
st = Store.empty(sa.n + sd.n, dev)
spare = Store.empty(sa.n + sd.n, dev)
ca = a["ctx"]
sc = Context.empty(ca[0], len(ca[1]) + len(d["ctx"][1]), dev)
rows = Store.empty(4 * nk, dev)
ctx_out = Context.empty(ca[0], sc.cap, dev)
changed = torch.empty(nk, dtype=torch.int64, device=dev)
ov, nv, fl, diffs = eng._diffs(nk)
rk = [torch.empty(nk, dtype=torch.int64, device=dev) for _ in range(4)]  # the two reads' keys and values
P = lambda t: C.cast(C.c_void_p(t.data_ptr()), _abi.P64)  # noqa: E731


def restore():
    for f in ("key", "val", "ts", "node", "cnt"):
        getattr(st, f)[: sa.n].copy_(getattr(sa, f)[: sa.n])
    st.n = sa.n
    sc.node[: len(ca[1])].copy_(torch.from_numpy(ca[1].view(np.int32)))
    sc.cnt[: len(ca[1])].copy_(torch.from_numpy(ca[2].view(np.int64)))
    sc.n = len(ca[1])
    t = ta.clone()
    t.store = st
    eng._order()
    torch.cuda.synchronize()
    return t


def fused():
    t = restore()  # (raw C-ABI calls on both sides: no wrapper's bookkeeping in either time)
    ss, xc, xd, cdx, sp, ro, co, tt = (st.abi(), sc.abi(), sd.abi(), cd.abi(), spare.abi(), rows.abi(),
                                       ctx_out.abi(), t.abi())
    nch, sw = C.c_uint64(), C.c_int()
    t0 = time.perf_counter()
    _abi.check(lib.dg_join_delta_diffs(eng.h, C.byref(ss), C.byref(xc), C.byref(xd), C.byref(cdx), P(keys), nk,
                                       C.byref(sp), C.byref(tt), P(changed), nk, C.byref(nch), C.byref(sw),
                                       C.byref(ro), C.byref(co), C.byref(diffs)))
    dt = time.perf_counter() - t0
    assert not sw.value
    m = nch.value
    return dt, (u64(changed[:m]).copy(), u64(ov[:m]).copy(), u64(nv[:m]).copy(), fl[:m].cpu().numpy().copy(),
                bool(sw.value))


def three_calls(reads=True):
    t = restore()
    ss, xc, xd, cdx, sp, ro, co, tt = (st.abi(), sc.abi(), sd.abi(), cd.abi(), spare.abi(), rows.abi(),
                                       ctx_out.abi(), t.abi())
    n0, n1, nch, sw = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    t0 = time.perf_counter()
    if reads:
        _abi.check(lib.dg_read_lww(eng.h, C.byref(ss), P(keys), nk, P(rk[0]), P(rk[1]), nk, C.byref(n0)))
    _abi.check(lib.dg_join_delta_out(eng.h, C.byref(ss), C.byref(xc), C.byref(xd), C.byref(cdx), P(keys), nk,
                                     C.byref(sp), C.byref(tt), P(changed), nk, C.byref(nch), C.byref(sw),
                                     C.byref(ro), C.byref(co)))
    if reads:
        _abi.check(lib.dg_read_lww(eng.h, C.byref(ss), P(changed), nch.value, P(rk[2]), P(rk[3]), nk, C.byref(n1)))
    dt = time.perf_counter() - t0
    assert not sw.value  # (config 4 joins in place: `st` keeps its columns)
    if not reads:
        return dt, None
    ch = u64(changed[: nch.value]).copy()
    ok, okv = u64(rk[0][: n0.value]), u64(rk[1][: n0.value])
    nk_, nkv = u64(rk[2][: n1.value]), u64(rk[3][: n1.value])
    # the caller's merge of the two reads into the three arrays (untimed)
    out = []
    for k, v in ((ok, okv), (nk_, nkv)):
        pos = np.minimum(np.searchsorted(k, ch), max(len(k) - 1, 0))
        has = (k[pos] == ch) if len(k) else np.zeros(len(ch), bool)
        out += [np.where(has, v[pos] if len(k) else 0, 0).astype(np.uint64), has]
    return dt, (ch, out[0], out[2], (out[1] * 1 + out[3] * 2).astype(np.uint8), bool(sw.value))


def join_only():  # dg_join_delta_out alone: what the diffs add to the call
    return three_calls(reads=False)


for f in (fused, three_calls, join_only):  # warm-up: code objects, scratch buffers
    f()
times = {"fused": [], "three_calls": [], "join_only": []}
res = {}
for _ in range(reps):
    for name, f in (("fused", fused), ("three_calls", three_calls), ("join_only", join_only)):
        dt, res[name] = f()
        times[name].append(dt * 1e6)
same = all(np.array_equal(x, y) for x, y in zip(res["fused"][:4], res["three_calls"][:4]))
print(f"config-4 shard: {sa.n} rows, {nk} keyset keys, {len(res['fused'][0])} changed, swapped "
      f"{res['fused'][4]}, results equal: {same}")
for name, t in times.items():
    t = np.sort(t)
    print(f"{name:12s} us per call: median {np.median(t):8.1f}  min {t[0]:8.1f}  max {t[-1]:8.1f}  ({reps} reps, alternating)")
assert same
