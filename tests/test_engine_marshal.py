"""The binding's three protocols with include/deltagpu.h, checked on the CPU: how `Engine`
marshals a list of keysets, how it commits a resident join, and how it answers
DG_E_CAPACITY.  The real `Engine` methods run against a stub that records every `dg_*` call
and writes results through the `byref` arguments, as the library would; stores and contexts
are CPU tensors, so no GPU and no built library are needed.
"""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from delta_crdt_ex_amd import _abi
from delta_crdt_ex_amd.store import Context, Engine, MerkleCont, MerkleTree, Store

CPU = torch.device("cpu")
COLS = ("key", "val", "ts", "node", "cnt")
U64_MAX = (1 << 64) - 1
CAPACITY = _abi.DG_E_CAPACITY


class StubLib:
    """Stands in for libdeltagpu: records (name, args) of every call and answers with the
    handler set for that entry point (default: DG_OK, nothing written)."""

    def __init__(self):
        self.calls = []
        self.on = {"dg_host_alloc": self._host_alloc}
        self.home = (C.c_uint64 * _abi.DG_HOME_DIFFS_WORDS)()

    def _host_alloc(self, h, nbytes, p):
        assert nbytes <= C.sizeof(self.home)
        p._obj.value = C.addressof(self.home)
        return 0

    def __getattr__(self, name):
        if not name.startswith("dg_"):
            raise AttributeError(name)

        def f(*args):
            self.calls.append((name, args))
            handler = self.on.get(name)
            return handler(*args) if handler else 0
        return f

    def named(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def eng(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_abi, "_lib", lib)  # check() asks it for dg_last_error
    e = Engine.__new__(Engine)
    e.lib, e.h, e.device, e.stream = lib, C.c_void_p(1), CPU, None
    e._order = lambda: None
    return e


def store(n=0, cap=8):
    s = Store.empty(cap, CPU)
    s.n = n
    return s


def context(n=0, cap=8):
    c = Context.empty(_abi.DG_CTX_VV, cap, CPU)
    c.n = n
    return c


def i64(n):
    return torch.arange(n, dtype=torch.int64)


def null(p):
    """A NULL pointer argument: None, or a ctypes pointer that holds no address."""
    return p is None or not bool(p)


def columns(s):
    return [getattr(s, f) for f in COLS]


def same(xs, ys):
    return all(x is y for x, y in zip(xs, ys))


# ------------------------------------------------------------------ keyset lists
# (entry point, index of k, of the pointer array, of the counts) in the C call
KEYSET_CALLS = {
    "apply_deltas": ("dg_apply_deltas", 3, 6, 7),
    "prepare_apply_deltas": ("dg_apply_deltas", 3, 6, 7),
    "join_deltas": ("dg_join_deltas", 3, 6, 7),
    "join_deltas_keyed": ("dg_join_deltas_keyed", 3, 6, 7),
    "take_keysets": ("dg_take_keysets", 2, 3, 4),
}


def run_keysets(eng, method, keys, k):
    """Call `method` with k deltas (or the keysets themselves) and return what the library
    saw, read while the call runs: (k, pointers or None, counts or None)."""
    name, ik, ikp, ikn = KEYSET_CALLS[method]
    seen = []

    def handler(*args):
        n, kp, kn = args[ik], args[ikp], args[ikn]
        seen.append((n, None if null(kp) else [kp[i] or 0 for i in range(n)],
                     None if null(kn) else [int(kn[i]) for i in range(n)]))
        return 0
    eng.lib.on[name] = handler
    state, sc, spare = store(4, 64), context(1), store(0, 64)
    deltas, dctxs = [store(1) for _ in range(k)], [context(1) for _ in range(k)]
    if method == "apply_deltas":
        eng.apply_deltas(state, sc, deltas, dctxs, keys)
    elif method == "prepare_apply_deltas":
        eng.prepare_apply_deltas(state, sc, deltas, dctxs, keys, store(0, 64), context(0, 64))()
    elif method == "take_keysets":
        eng.take_keysets(state, keys)
    else:
        getattr(eng, method)(state, sc, deltas, dctxs, keys, spare)
    assert len(seen) == 1
    return seen[0]


@pytest.mark.parametrize("method", list(KEYSET_CALLS))
def test_keyset_list(eng, method):
    """None -> NULL (every key); an empty tensor -> a valid pointer with n = 0 (no key);
    a tensor -> its address and length."""
    empty, three = torch.zeros(0, dtype=torch.int64), i64(3)
    keys = [empty, three] if method == "take_keysets" else [None, empty, three]
    k, kp, kn = run_keysets(eng, method, keys, len(keys))
    assert k == len(keys)
    if method != "take_keysets":
        assert kp[0] == 0 and kn[0] == 0
    assert kp[-2] != 0 and kn[-2] == 0
    assert kp[-1] == three.data_ptr() and kn[-1] == 3


@pytest.mark.parametrize("method", [m for m in KEYSET_CALLS if m != "take_keysets"])
def test_keyset_list_none(eng, method):
    k, kp, kn = run_keysets(eng, method, None, 2)
    assert k == 2 and kp is None and kn is None


@pytest.mark.parametrize("method", list(KEYSET_CALLS))
def test_keyset_list_of_none(eng, method):
    k, _, _ = run_keysets(eng, method, [], 0)
    assert k == 0


# ------------------------------------------------------------------ join commit
# per entry point the argument indices of (state, state ctx, spare, tree, n changed, swapped,
# rows, ctx_out, diffs); None: the entry point has no such argument
JOIN_ARGS = {
    "dg_join_delta_rows": (1, 2, 7, 8, 11, 12, 13, None, None),
    "dg_join_delta_diffs": (1, 2, 7, 8, 11, 12, 13, 14, 15),
    "dg_join_deltas": (1, 2, 8, 9, 12, None, 13, 14, 15),
    "dg_join_deltas_keyed": (1, 2, 8, 9, 12, 16, 13, 14, 15),
    "dg_join_delta_home": (1, 2, 7, 8, None, 10, None, None, None),
    "dg_join_delta_home_diffs": (1, 2, 7, 8, None, 10, None, None, None),
}
JOIN_ENTRY = {"join_delta": "dg_join_delta_rows", "join_delta_diffs": "dg_join_delta_diffs",
              "join_deltas": "dg_join_deltas", "join_deltas_keyed": "dg_join_deltas_keyed",
              "join_delta_home": "dg_join_delta_home"}


def join_writer(name, swapped, n_changed=2, diffs_cap=None, home0=0):
    """A handler that answers a resident join as the library does: the new counts in the
    structs, the swapped flag, and (home calls) the head of the page-locked block."""
    iss, isc, isp, it, inn, isw, iro, ico, idf = JOIN_ARGS[name]

    def handler(*a):
        a[iss]._obj.n, a[isc]._obj.n, a[isc]._obj.kind = 7, 5, _abi.DG_CTX_DOTS
        a[isp]._obj.n = 9
        a[it]._obj.n_keys = U64_MAX
        if inn is not None:
            a[inn]._obj.value = n_changed
        if isw is not None:
            a[isw]._obj.value = int(swapped)
        if iro is not None and a[iro] is not None:
            a[iro]._obj.n = 3
        if ico is not None and a[ico] is not None:
            a[ico]._obj.n, a[ico]._obj.kind = 4, _abi.DG_CTX_DOTS
        if idf is not None and diffs_cap is not None:
            a[idf]._obj.cap = diffs_cap
        if "home" in name:
            home = C.cast(a[9], C.POINTER(C.c_uint64))
            home[0], home[1], home[2], home[3] = home0, 1, 1, 1
        return 0
    return handler


class Replica:
    """A resident state on the CPU with what a join of it needs, and what it looked like
    before the join."""

    def __init__(self):
        self.state, self.ctx, self.spare = store(6, 16), context(2), store(0, 16)
        self.tree = MerkleTree.empty(4, CPU)
        self.tree.store = self.state
        self.rows, self.ctx_out = store(0, 16), context(0, 16)
        self.state_cols, self.spare_cols = columns(self.state), columns(self.spare)
        self.before = [dict(vars(x)) for x in (self.state, self.ctx, self.spare, self.tree)]

    def unchanged(self):
        now = [dict(vars(x)) for x in (self.state, self.ctx, self.spare, self.tree)]
        return all(a.keys() == b.keys() and all(a[f] is b[f] or (isinstance(a[f], int) and a[f] == b[f])
                                                for f in a) for a, b in zip(now, self.before))

    def join(self, eng, method, k=2, **kw):
        delta, dctx, keys = store(2), context(1), i64(3)
        head = (self.state, self.ctx)
        if method in ("join_deltas", "join_deltas_keyed"):
            return getattr(eng, method)(*head, [store(2) for _ in range(k)], [context(1) for _ in range(k)],
                                        [keys] * k, self.spare, self.tree, rows=self.rows,
                                        ctx_out=self.ctx_out, **kw)
        if method == "join_delta":
            self.ctx_out = None
            return eng.join_delta(*head, delta, dctx, keys, self.spare, self.tree, rows=self.rows)
        if method == "join_delta_diffs":
            return eng.join_delta_diffs(*head, delta, dctx, keys, self.spare, self.tree, rows=self.rows,
                                        ctx_out=self.ctx_out, **kw)
        self.rows = self.ctx_out = None
        return getattr(eng, method)(*head, delta, dctx, keys, self.spare, self.tree)


@pytest.mark.parametrize("swapped", [True, False])
@pytest.mark.parametrize("method", list(JOIN_ENTRY))
def test_join_commit(eng, method, swapped):
    name = JOIN_ENTRY[method]
    # dg_join_deltas has no swapped flag: it goes through the spare exactly when it has a delta
    k = 0 if method == "join_deltas" and not swapped else 2
    eng.lib.on[name] = join_writer(name, swapped, n_changed=k)
    r = Replica()
    res = r.join(eng, method, k=k)
    assert len(eng.lib.named(name)) == 1
    if swapped:
        assert same(columns(r.state), r.spare_cols) and same(columns(r.spare), r.state_cols)
        assert r.spare.n == 0
    else:
        assert same(columns(r.state), r.state_cols) and same(columns(r.spare), r.spare_cols)
    assert (r.state.n, r.ctx.n, r.ctx.kind) == (7, 5, _abi.DG_CTX_DOTS)
    if r.rows is not None:
        assert r.rows.n == 3
    if r.ctx_out is not None:
        assert (r.ctx_out.n, r.ctx_out.kind) == (4, _abi.DG_CTX_DOTS)
    assert r.tree.n_keys == U64_MAX
    assert r.tree.store is r.state
    assert res[-1] is swapped
    if method != "join_delta_home":
        assert res[0].numel() == k


def test_join_delta_diffs_ungathered(eng):
    """The library reports its diffs were not gathered (cap 0 with changed keys): the old rows
    are read from the spare, which holds its rows while that read runs and none afterwards;
    a join that went in place has overwritten them."""
    eng.lib.on["dg_join_delta_diffs"] = join_writer("dg_join_delta_diffs", True, diffs_cap=0)
    r = Replica()
    res = r.join(eng, "join_delta_diffs")
    (read,) = eng.lib.named("dg_read_diff")
    assert read[1]._obj.n == 9 and read[1]._obj.key == r.state_cols[0].data_ptr()  # old: the spare
    assert read[2]._obj.n == 7 and read[2]._obj.key == r.spare_cols[0].data_ptr()  # new: the state
    assert r.spare.n == 0 and res[-1] is True and res[1].numel() == 2
    eng.lib.on["dg_join_delta_diffs"] = join_writer("dg_join_delta_diffs", False, diffs_cap=0)
    with pytest.raises(_abi.DeltaGpuError, match="old rows are overwritten"):
        Replica().join(eng, "join_delta_diffs")


# ------------------------------------------------------------------ declines
def test_keyed_join_declined(eng):
    eng.lib.on["dg_join_deltas_keyed"] = lambda *a: _abi.DG_KEYED_FALLBACK
    r = Replica()
    assert r.join(eng, "join_deltas_keyed") is None
    assert r.unchanged()


@pytest.mark.parametrize("method", ["join_delta_home", "join_delta_home_diffs"])
def test_home_join_declined(eng, method):
    name = "dg_" + method
    eng.lib.on[name] = join_writer(name, False, home0=_abi.DG_HOME_FALLBACK)
    assert Replica().join(eng, method) is None


# ------------------------------------------------------------------ capacity retries
def test_take_keys_retry(eng):
    caps = []

    def handler(h, ss, kp, nk, so):
        caps.append(so._obj.cap)
        so._obj.n = 900
        return CAPACITY if len(caps) == 1 else 0
    eng.lib.on["dg_take_keys"] = handler
    out = eng.take_keys(store(5000, 5000), i64(3))
    assert caps == [256, 5000]  # four rows per key (256 at least), then the store's size
    assert out.n == 900 and out.cap == 5000


def take_keysets_handler(seen):
    def handler(h, ss, k, kp, kn, ukeys, masks, offs, cap_keys, nu, so):
        seen.append((cap_keys, so._obj.cap))
        nu._obj.value, so._obj.n = 10, 700
        return CAPACITY if cap_keys < 10 or so._obj.cap < 700 else 0
    return handler


def test_take_keysets_retry(eng):
    seen = []
    eng.lib.on["dg_take_keysets"] = take_keysets_handler(seen)
    ukeys, masks, offs, out = eng.take_keysets(store(5000, 5000), [i64(3), i64(1)])
    assert seen == [(4, 256), (10, 700)]
    assert (ukeys.numel(), masks.numel(), offs.numel(), out.n) == (10, 10, 11, 700)


def test_take_keysets_callers_buffers(eng):
    seen = []
    eng.lib.on["dg_take_keysets"] = take_keysets_handler(seen)
    with pytest.raises(_abi.CapacityError) as err:
        eng.take_keysets(store(5000, 5000), [i64(3), i64(1)], out=store(0, 8), cap_keys=4)
    assert seen == [(4, 8)]
    assert (err.value.n_ukeys, err.value.n_rows) == (10, 700)


def test_mutate_batch_retry(eng):
    caps = []

    def handler(*a):
        caps.append(a[12]._obj.cap)
        a[11]._obj.n, a[12]._obj.n, a[12]._obj.kind, a[15]._obj.value = 2, 3, _abi.DG_CTX_DOTS, 1
        return CAPACITY if len(caps) == 1 else 0
    eng.lib.on["dg_mutate_batch"] = handler
    m, n_adds, state = 2, 1, store(100, 128)
    out, dots, keys = eng.mutate_batch(state, context(1), 5, torch.ones(m, dtype=torch.uint8), i64(m), i64(m),
                                       i64(m), i64(m), n_adds)
    assert caps == [8 * m + n_adds + 1, state.n + n_adds + 1]
    assert (out.n, dots.n, dots.kind, dots.cap, keys.numel()) == (2, 3, _abi.DG_CTX_DOTS, caps[1], 1)


def cont_of(n):
    c = MerkleCont.empty(max(n, 1), 1, CPU)
    c.level, c.n = 2, n
    return c


def tree_over(s):
    t = MerkleTree.empty(4, CPU)
    t.store = s
    return t


@pytest.mark.parametrize("method,ico", [("merkle_continue", 5), ("merkle_continue_home", 6)])
def test_merkle_continue_retry(eng, method, ico):
    caps = []

    def handler(*a):
        co = a[ico]._obj
        caps.append((co.cap, co.cap_buckets))
        co.level, co.n, co.n_buckets = 3, 100, 50
        a[-1]._obj.value = 1  # a continuation
        return CAPACITY if len(caps) == 1 else 0
    eng.lib.on["dg_" + method] = handler
    status, out = getattr(eng, method)(tree_over(store(20, 32)), cont_of(2))
    assert caps[0] == (8, 2) and len(caps) == 2
    assert caps[1][0] >= 100 and caps[1][1] >= 50
    assert status == "continue" and (out.level, out.n, out.n_buckets) == (3, 100, 50)


def hops_handler(seen, take):
    """Answers dg_merkle_continues[_take]: the hop whose input has 2 entries needs an output of
    (64, 32); with `take`, the rows of the hop whose input has 1 entry need 999."""
    def handler(*a):
        n, batch, tptr = a[3], a[4], a[5] if take else None
        call = []
        for i in range(n):
            h = batch[i]
            cin, co = h.in_.contents, h.out.contents
            rows = tptr[i].contents if take and tptr[i] else None
            call.append((cin.n, co.cap, co.cap_buckets, rows.rows.cap if rows else None))
            h.rc, h.status, h.n_keys, h.n_total = 0, 0, 2, 5
            if cin.n == 2 and (co.cap < 64 or co.cap_buckets < 32):
                h.rc, co.n, co.n_buckets = CAPACITY, 64, 32
            elif rows is not None:
                rows.rc, rows.rows.n = (CAPACITY, 999) if rows.rows.cap < 999 else (0, 999)
        seen.append(call)
        return 0
    return handler


def test_merkle_continues_retry(eng):
    seen = []
    eng.lib.on["dg_merkle_continues"] = hops_handler(seen, False)
    res = eng.merkle_continues(tree_over(store(20, 32)), [cont_of(1), cont_of(2), cont_of(3)])
    assert [c[0] for c in seen[0]] == [1, 2, 3]
    assert len(seen) == 2 and len(seen[1]) == 1  # only the hop that reported capacity again
    n, cap, bcap, _ = seen[1][0]
    assert n == 2 and cap >= 64 and bcap >= 32
    assert [r[0] for r in res] == ["ok"] * 3 and all(r[1].numel() == 2 and r[2] == 5 for r in res)
    assert not eng.lib.named("dg_merkle_continues_take")


def test_merkle_continues_no_retry(eng):
    seen = []
    eng.lib.on["dg_merkle_continues"] = hops_handler(seen, False)
    res = eng.merkle_continues(tree_over(store(20, 32)), [cont_of(1), cont_of(2), cont_of(3)], retry=False)
    assert len(seen) == 1
    assert res[1] == ("capacity", 64, 32) and res[0][0] == res[2][0] == "ok"


def test_merkle_continues_take_retry(eng):
    seen = []
    eng.lib.on["dg_merkle_continues_take"] = hops_handler(seen, True)
    res = eng.merkle_continues_take(tree_over(store(5000, 5000)), [cont_of(1), cont_of(2), cont_of(3)],
                                    [True, True, False], row_caps=[100, None, None])
    assert [c[0] for c in seen[0]] == [1, 2, 3]
    assert seen[0][0][3] == 100 and seen[0][2][3] is None  # the caller's size; no rows asked
    assert len(seen) == 2 and [c[0] for c in seen[1]] == [1, 2]  # the short take, the short hop
    assert seen[1][0][3] == 999 and seen[1][1][1] >= 64 and seen[1][1][2] >= 32
    assert len(res[0]) == 5 and res[0][3].numel() == 3 and res[0][4].n == 999
    assert len(res[1]) == 5 and len(res[2]) == 3
    assert not eng.lib.named("dg_merkle_continues")


def test_merkle_continues_take_no_retry(eng):
    seen = []
    eng.lib.on["dg_merkle_continues_take"] = hops_handler(seen, True)
    res = eng.merkle_continues_take(tree_over(store(5000, 5000)), [cont_of(1), cont_of(2), cont_of(3)],
                                    [True, True, False], row_caps=[100, None, None], retry=False)
    assert len(seen) == 1
    assert res[0][:1] + res[0][2:] == ("ok", 5, None, ("capacity", 999)) and res[0][1].numel() == 2
    assert res[1] == ("capacity", 64, 32)
    assert res[2][0] == "ok" and len(res[2]) == 3
