"""bench.py --dump-outputs: the files hold the join's rows and context exactly (64-bit
columns as their 32-bit halves in float64), the row sample is fixed by the row count,
and the whole-column checksums are exact.  Checked against the C oracle's join."""
import numpy as np
import pytest

import bench
from delta_crdt_ex_amd import workloads as W
from oracle import ref as R


def _u64(h):
    return (h[:, 0].astype(np.uint64) << np.uint64(32)) | h[:, 1].astype(np.uint64)


def test_halves_and_piece_sums_are_exact():
    x = np.array([0, 1, 2**32 - 1, 2**32, 2**53 + 1, 2**64 - 1], dtype=np.uint64)
    h = bench._halves(x)
    assert h.dtype == np.float64 and h.shape == (6, 2)
    assert np.array_equal(_u64(h), x)
    assert np.array_equal(_u64(bench._halves(np.array([-1, -2**63], dtype=np.int64))),
                          np.array([2**64 - 1, 2**63], dtype=np.uint64))
    s = bench._piece_sums(x)
    want = [sum((int(v) >> sh) & 0xFFFF for v in x) for sh in (0, 16, 32, 48)]
    assert s == [float(w) for w in want]
    assert bench._piece_sums(np.array([2**32 - 1], dtype=np.uint32)) == [65535.0, 65535.0, 0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [None, 1000])
def test_dump_outputs_equals_the_oracle_join(engine, tmp_path, monkeypatch, cap):
    import torch

    from delta_crdt_ex_amd.store import Context, Store
    if cap:
        monkeypatch.setattr(bench, "DUMP_ROWS", cap)
    dev = "cuda:0"
    a, b = W.config2(n_keys=5000, seed=11)
    sa, sb = Store.from_numpy(*a["rows"], device=dev), Store.from_numpy(*b["rows"], device=dev)
    ca, cb = Context.from_numpy(*a["ctx"], dev), Context.from_numpy(*b["ctx"], dev)
    out, octx = Store.empty(sa.n + sb.n, dev), Context.empty(0, ca.n + cb.n, dev)
    d = torch.zeros(8, dtype=torch.int64, device=dev)
    pr = dict(out=out, octx=octx, d=d, launch=engine.prepare_join2(sa, ca, sb, cb, out, octx, d))
    pr["launch"]()
    engine.sync()
    for _ in range(2):  # the same files whenever it is called
        bench.dump_outputs(str(tmp_path), pr, 0, 1)
    rows, ctx = R.join2(a["rows"], a["ctx"], b["rows"], b["ctx"])
    n = len(rows[0])
    load = lambda f: np.load(tmp_path / f"{f}.npy")  # noqa: E731
    for f in ("counts", "rows_index", "rows_checksum", "rows_key", "rows_node", "ctx_cnt"):
        assert load(f).dtype == np.float64
    assert load("counts").tolist() == [n, len(ctx[1]), ctx[0]]
    idx = load("rows_index").astype(np.int64)
    if cap:
        assert n > cap and len(idx) == cap and np.all(np.diff(idx) > 0) and idx[-1] < n
        assert np.array_equal(idx, np.sort(np.random.default_rng(0).choice(n, cap, replace=False)))
    else:
        assert np.array_equal(idx, np.arange(n))
    for f, c in zip(("key", "val", "ts", "node", "cnt"), rows):
        got = load(f"rows_{f}")
        got = got.astype(np.uint32) if f == "node" else _u64(got)
        assert np.array_equal(got, c[idx].view(got.dtype)), f
    want = [bench._piece_sums(c.view(np.uint32 if c.dtype.itemsize == 4 else np.uint64)) for c in rows]
    assert np.array_equal(load("rows_checksum"), np.array(want))
    assert np.array_equal(load("ctx_node").astype(np.uint32), ctx[1])
    assert np.array_equal(_u64(load("ctx_cnt")), ctx[2])
