"""dg_mark_ids against its yardstick, dg_remap_values as an identity remap, and dgr_sweep's
wall time (profiles/sweep.txt).

The stores are one 1M-key config-2 replica and one 12.5M-key config-5 share (--small: 100k /
1M keys).  For the value column the store's val column is replaced by draws from the table, so
that every row holds a table value: the remap then reads the same bytes and does the same
search as the mark, and also writes 8 B per row.  The two calls alternate in one process;
each is timed with device events on the engine stream (the whole launch chain of the call).
Algorithmic bytes of the mark: 8 per row + 9 per id (the table read once, one flag byte out).

    python tools/prof_sweep.py                 # the timings
    python tools/prof_sweep.py --calls 10      # 10 value-column mark calls only (a trace target)
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from delta_crdt_ex_amd import _abi, nif  # noqa: E402
from delta_crdt_ex_amd import workloads as W  # noqa: E402
from delta_crdt_ex_amd.interning import splitmix64_np  # noqa: E402
from delta_crdt_ex_amd.store import Engine, Store  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (spec)
REPS, WARM = 15, 3


def value_table(n, seed):
    """n ascending non-canonical value ids (the HIGH region)"""
    x = splitmix64_np(np.arange(1, 2 * n + 64, dtype=np.uint64) ^ np.uint64(seed)) | np.uint64(1 << 63)
    return np.unique(x)[:n]


def timed(eng, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def stats(v):
    v = np.array(v[WARM:])
    return float(np.median(v)), float(v.min()), float(v.max())


def fmt(name, v, nbytes=None):
    med, lo, hi = stats(v)
    s = f"{name:34s} median {med:9.1f} us  min {lo:9.1f}  max {hi:9.1f}"
    if nbytes is not None:
        s += f"  {nbytes / med / 1e6:7.2f} TB/s = {100 * nbytes / (med * 1e-6) / HBM_PEAK:5.1f} % of HBM peak"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--calls", type=int, default=0)
    a = ap.parse_args()
    dev = "cuda:0"
    eng = Engine(0)
    lib = eng.lib
    print("build digest", lib.dg_build_digest().decode(), "device", torch.cuda.get_device_name(0))
    n2, n5 = (100_000, 1_000_000) if a.small else (1_000_000, 12_500_000)
    shapes = [("config-2 replica", W.config2(n_keys=n2)[0])]
    if not a.calls:
        shapes.append(("config-5 share", W.config5_shard(0, 8, keys_per_rank=n5)[0]))
    c2_rows = shapes[0][1]["rows"]
    for name, rep in shapes:
        key, _val, ts, node, cnt = rep["rows"]
        rows = len(key)
        print(f"== {name}: {rows} rows, {len(np.unique(key))} keys")
        for n_ids in (2048, 100_000, 1_000_000) if not a.small else (2048, 100_000):
            ids = value_table(n_ids, 7)
            val = ids[(splitmix64_np(np.arange(rows, dtype=np.uint64)) % np.uint64(n_ids)).astype(np.int64)]
            st = Store.from_numpy(key, val, ts, node, cnt, dev)
            d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
            used = torch.empty(n_ids, dtype=torch.uint8, device=dev)
            arr = (_abi.dg_store * 1)(st.abi())
            nu, nx = C.c_uint64(), C.c_uint64()
            idp = C.cast(C.c_void_p(d_ids.data_ptr()), _abi.P64)
            torch.cuda.synchronize()

            def mark():
                _abi.check(lib.dg_mark_ids(eng.h, arr, 1, _abi.DG_COL_VAL, idp, n_ids,
                                           C.c_void_p(used.data_ptr()), C.byref(nu), C.byref(nx)))

            def remap():
                _abi.check(lib.dg_remap_values(eng.h, C.byref(arr[0]), idp, idp, n_ids))

            if a.calls:
                for _ in range(a.calls):
                    mark()
                print(f"{a.calls} dg_mark_ids calls, table {n_ids}: n_used {nu.value} unknown {nx.value}")
                continue
            tm, tr = [], []
            for _ in range(REPS + WARM):
                tm.append(timed(eng, mark))
                tr.append(timed(eng, remap))
            assert nx.value == 0 and nu.value == len(np.unique(val))
            nbytes = 8 * rows + 9 * n_ids
            print(f"-- value column, table of {n_ids} ids ({nu.value} used)")
            print(fmt("dg_mark_ids", tm, nbytes))
            print(fmt("dg_remap_values (identity)", tr, nbytes + 8 * rows))
            mm, mr = stats(tm)[0], stats(tr)
            print(f"   mark / remap medians = {mm / mr[0]:.3f}; remap's own spread (max - min) / median = "
                  f"{(mr[2] - mr[1]) / mr[0]:.3f}")
        if a.calls:
            continue
        # the key column: the store's keys plus a quarter as many dead ids (the windowed search)
        uk = np.unique(key)
        dead = splitmix64_np(np.arange(len(uk) // 4, dtype=np.uint64) ^ np.uint64(0xDEAD))
        ids = np.unique(np.concatenate([uk, dead]))
        st = Store.from_numpy(key, _val, ts, node, cnt, dev)
        d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
        used = torch.empty(len(ids), dtype=torch.uint8, device=dev)
        arr = (_abi.dg_store * 1)(st.abi())
        nu, nx = C.c_uint64(), C.c_uint64()
        idp = C.cast(C.c_void_p(d_ids.data_ptr()), _abi.P64)
        torch.cuda.synchronize()
        tk = [timed(eng, lambda: _abi.check(lib.dg_mark_ids(eng.h, arr, 1, _abi.DG_COL_KEY, idp, len(ids),
                                                            C.c_void_p(used.data_ptr()), C.byref(nu),
                                                            C.byref(nx))))
              for _ in range(REPS + WARM)]
        assert nx.value == 0 and nu.value == len(uk)
        print(f"-- key column, table of {len(ids)} ids ({nu.value} used), windowed search")
        print(fmt("dg_mark_ids", tk, 8 * rows + 9 * len(ids)))
    if a.calls:
        return
    # dgr_sweep's wall time: upload of the table, the mark over the state, the flags home
    g = nif.Engine(0)
    key, val, ts, node, cnt = c2_rows
    n_ids = 100_000 if a.small else 1_000_000
    ids = value_table(n_ids, 9)
    val = np.ascontiguousarray(ids[(splitmix64_np(np.arange(len(key), dtype=np.uint64)) % np.uint64(n_ids // 2))
                                   .astype(np.int64)])  # half of the table is dead
    hs = _abi.dg_store(key.ctypes.data, val.ctypes.data, ts.ctypes.data, node.ctypes.data, cnt.ctypes.data,
                       len(key), len(key))
    cn, cc = np.zeros(1, np.uint32), np.array([1 << 40], np.uint64)
    hc = _abi.dg_context(_abi.DG_CTX_VV, 0, cn.ctypes.data, cc.ctypes.data, 1, 1)
    sp = C.c_void_p()
    _abi.check(g.lib.dgr_state_load(g.ptr, C.byref(hs), C.byref(hc), C.byref(sp)))
    wall = []
    for _ in range(REPS + WARM):
        t0 = time.perf_counter()
        rc, used, unknown = g._mark(_abi.DG_COL_VAL, ids)
        wall.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0 and unknown == 0
    assert int(used.sum()) == len(np.unique(val))
    print(f"== dgr_sweep (value column): {len(key)}-row state, table of {n_ids} ids, {int(used.sum())} used")
    print(fmt("dgr_sweep wall (incl. flag copy-out)", wall))
    g.lib.dgr_state_free(sp)
    g.close()
    eng.close()


if __name__ == "__main__":
    main()
