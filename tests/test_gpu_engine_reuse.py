"""One engine reused across sizes and tree depths: the engine's scratch grows on demand
(csrc/api_engine.hip grow) and every call carves its layout from whatever buffer is there
(csrc/dg_arena.h), so a call after a larger one runs in a larger buffer, a call after a
smaller one regrows it, and dg_join_delta's zero-between-calls buffer must still be zero
after it regrew.  Small, large, small again -- on each of dg_join_delta's three paths (the
one-wait path; DG_KD=0: the splice; DG_SPLICE=0 too: the full join), then the home join, a
two-step dg_joink and dg_mutate_batch on the same engine.  Every result against the C
oracle, every tree against a fresh build (apply)."""
import functools

import numpy as np
import pytest

from delta_crdt_ex_amd import workloads as W
from delta_crdt_ex_amd.store import Engine, u64
from kfold_cases import random_fold
from oracle import ref as R
from test_gpu_join_delta import apply
from test_gpu_mutate import random_ops, run as mutate
from test_gpu_parity import ctx_eq, rows_eq, up

pytestmark = pytest.mark.gpu

# (state keys, delta keys): a few hundred keys, a few thousand, a few hundred again.  The
# states are large enough against their deltas for the splice to apply (8 rows per delta
# row and key).
SMALL, LARGE = (8_000, 200), (80_000, 2_000)
# depth 8 and 12: one and two chunks; 18 (128 chunks) is past the 256 bytes the zeroed
# buffer starts with, so it regrows between calls
STEPS = [(8, SMALL), (12, LARGE), (18, LARGE), (8, SMALL)]


@functools.lru_cache(maxsize=None)
def _sync_case(n_state, n_keys):
    rng = np.random.default_rng(n_state + n_keys)
    a, b = W.random_pair(rng, n_state, n_nodes=5, ts_range=1 << 10)
    kb = np.unique(np.concatenate([a["rows"][0], b["rows"][0]]))
    keys = np.sort(rng.choice(kb, n_keys, replace=False))
    return a, W.sync_delta(b, keys), keys


@pytest.mark.parametrize("path", ["one-wait", "splice", "full"])
def test_one_engine_across_sizes_and_depths(monkeypatch, path):
    monkeypatch.setenv("DG_KD", "1" if path == "one-wait" else "0")
    monkeypatch.setenv("DG_SPLICE", "0" if path == "full" else "1")
    eng = Engine(0)
    try:
        for depth, (n_state, n_keys) in STEPS:
            a, d, keys = _sync_case(n_state, n_keys)
            if path != "full":  # (the splice's own condition, so that DG_KD=0 does splice)
                assert (len(keys) + len(d["rows"][0])) * 8 <= len(a["rows"][0])
            apply(eng, a, d, keys, depth=depth)
        # the home join: at most 512 keys and delta rows, so the sizes are the states'
        for depth, n_state, n_keys in [(8, 2_000, 60), (12, 30_000, 120), (8, 2_000, 60)]:
            a, d, keys = _sync_case(n_state, n_keys)
            assert len(d["rows"][0]) <= 512
            apply(eng, a, d, keys, depth=depth, home=True)
        # a two-step dg_joink (three replicas: the ping-pong buffers)
        for n in (300, 3_000, 300):
            rng = np.random.default_rng(n)
            reps = [W.random_pair(rng, n_keys=n, ts_range=8)[i % 2] for i in range(3)]
            stores, ctxs = zip(*[up(r) for r in reps])
            out, octx = eng.joink(list(stores), list(ctxs))
            wr, wc = R.joink([r["rows"] for r in reps], [r["ctx"] for r in reps])
            rows_eq(out, wr)
            ctx_eq(octx, wc)
        # dg_mutate_batch
        st, _ = random_fold(90, n_keys=5000, k=0, n_nodes=6, rows_per_key=3)
        for n_ops in (300, 3_000, 300):
            ops = random_ops(np.random.default_rng(n_ops), np.unique(st["rows"][0]), n_ops)
            drows, dctx, dkeys = mutate(eng, st, 9, ops)
            wr, wc, wk = R.mutate_batch(st["rows"], st["ctx"], 9, ops)
            rows_eq(drows, wr)
            ctx_eq(dctx, wc)
            assert np.array_equal(u64(dkeys), wk)
    finally:
        eng.close()
