"""Universe.sweep (interning.py): pure host logic, no GPU.  The flags a real sweep gets from
the device (dg_mark_ids) are made up here."""
import numpy as np
import pytest

from delta_crdt_ex_amd import interning, storage
from delta_crdt_ex_amd.interning import CANON_LO, Universe
from delta_crdt_ex_amd.terms import Atom, order_key

# a term of every class the table orders: integers below CANON_LO, floats, atoms, tuples, binaries
CLASS_TERMS = [CANON_LO - 5, CANON_LO - 1, -2.5, 0.0, 3.75, Atom("ok"), Atom("zz"), (1, 2), ("a", 1.5),
               "bin", b"\x00\x01", "zebra"]


def _terms(n, seed=0):
    rng = np.random.default_rng(seed)
    out = list(CLASS_TERMS)
    rs = rng.permutation(1 << 20)[:n]  # distinct: no term twice
    for i in range(n):
        r = int(rs[i]) + 1
        out.append([f"s{r:08x}", r / 7.0, (r, f"t{i}"), Atom(f"a{r}"), CANON_LO - 10 - r][i % 5])
    return out


def _check_order(U):
    """every adjacent pair of value_ids() ascends in id and in terms.order_key order"""
    ids, terms = U.value_ids()
    assert len(ids) == U.value_count()
    for j in range(len(ids) - 1):
        assert ids[j] < ids[j + 1]
        assert order_key(terms[j]) < order_key(terms[j + 1]), (terms[j], terms[j + 1])


def _flags(U, live_terms):
    ids, terms = U.value_ids()
    live = {order_key(t) for t in live_terms}
    return np.array([order_key(t) in live for t in terms], np.uint8)


def test_survivors_keep_ids_terms_and_hashes_and_dropped_ids_raise():
    U = Universe()
    terms = _terms(400)
    vid = {i: U.value(t) for i, t in enumerate(terms)}
    canon = U.value(12345)  # a canonical integer: no table entry, nothing to sweep
    _nh, ids0, hash0 = U.term_tables()
    h0 = dict(zip(ids0.tolist(), hash0.tolist()))
    live = [t for i, t in enumerate(terms) if i % 3 == 0]
    epoch, version = U.val_epoch, U.terms_version
    out = U.sweep(_flags(U, live))
    assert out == {"values": (len(terms), len(live)), "keys": (0, 0)}
    assert U.value_count() == len(live)
    assert U.val_epoch == epoch and U.terms_version > version
    _nh, ids1, hash1 = U.term_tables()
    assert len(ids1) == len(live) and np.all(ids1[:-1] < ids1[1:])
    for i, t in enumerate(terms):
        if i % 3 == 0:
            assert U.value_term(vid[i]) == t and U.value(t) == vid[i]
            assert dict(zip(ids1.tolist(), hash1.tolist()))[vid[i]] == h0[vid[i]]
        else:
            with pytest.raises(KeyError):
                U.value_term(vid[i])
    assert U.value_term(canon) == 12345
    assert U.value_count() == len(live)  # looking the survivors up interned nothing
    _check_order(U)
    assert U.sweep(np.ones(len(live), np.uint8))["values"] == (len(live), len(live))  # nothing to drop


def test_keep_arguments_pin_unflagged_entries():
    U = Universe()
    terms = _terms(50)
    for t in terms:
        U.value(t)
    keys = ["k1", 7, (1, "x"), Atom("k")]
    kids = [U.key(k) for k in keys]
    assert U.key_count() == 4 and sorted(kids) == U.key_ids().tolist()
    pinned_v = [terms[3], terms[20]]
    out = U.sweep(np.zeros(U.value_count(), np.uint8), np.zeros(4, np.uint8), keep_values=pinned_v,
                  keep_keys=[keys[2]])
    assert out == {"values": (len(terms), 2), "keys": (4, 1)}
    assert sorted(map(order_key, U.value_ids()[1])) == sorted(map(order_key, pinned_v))
    assert U.key_term(kids[2]) == keys[2]
    for i in (0, 1, 3):
        with pytest.raises(KeyError):
            U.key_term(kids[i])
    assert U.key(keys[0]) == kids[0] and U.key_count() == 2  # interned afresh: the id is the term's hash


def test_flag_arrays_of_the_wrong_length_are_refused():
    U = Universe()
    for t in _terms(10):
        U.value(t)
    U.key("k")
    n = U.value_count()
    with pytest.raises(ValueError):
        U.sweep(np.ones(n - 1, np.uint8))
    with pytest.raises(ValueError):
        U.sweep(np.ones(n, np.uint8), np.ones(2, np.uint8))
    assert U.value_count() == n and U.key_count() == 1


def test_reinterned_dropped_terms_land_between_the_right_neighbours():
    U = Universe()
    terms = _terms(600, seed=1)
    for t in terms:
        U.value(t)
    _check_order(U)
    live = [t for i, t in enumerate(terms) if i % 3 == 1]  # drops every CLASS_TERMS member with i % 3 != 1
    U.sweep(_flags(U, live))
    _check_order(U)
    before = dict(zip(map(order_key, U.value_ids()[1]), U.value_ids()[0]))
    epoch = U.val_epoch
    for t in CLASS_TERMS + [t for i, t in enumerate(terms) if i % 3 == 2] + _terms(100, seed=2):
        U.value(t)
        _check_order(U)  # after every insert: the new id lies between its neighbours'
    for t in CLASS_TERMS:  # one term of each class is in the table again
        assert U.value_term(U.value(t)) == t
    if U.val_epoch == epoch:  # no relabel happened: the survivors' ids did not move
        now = dict(zip(map(order_key, U.value_ids()[1]), U.value_ids()[0]))
        assert all(now[k] == v for k, v in before.items())


def test_relabel_after_a_sweep_returns_survivors_only():
    U = Universe()
    terms = _terms(90)
    for t in terms:
        U.value(t)
    live = [t for t in terms if not isinstance(t, int)][1::2]  # the HIGH region's survivors
    low = [t for t in terms if isinstance(t, int)][:3]         # the LOW region's
    U.sweep(_flags(U, live + low))
    seen = []
    U.remap_hook = lambda old, new: seen.append((old.copy(), new.copy()))
    high_ids = [v for v in U.value_ids()[0] if v >= interning.CANON_ID_HI]
    low_ids = [v for v in U.value_ids()[0] if v < interning.CANON_ID_LO]
    assert len(low_ids) == 3
    old, new = U.relabel()
    assert old.tolist() == high_ids and len(new) == len(high_ids) == len(live)
    old, new = U.relabel(low=True)
    assert old.tolist() == low_ids
    assert [len(o) for o, _ in seen] == [len(high_ids), 3]
    _check_order(U)
    assert sorted(map(order_key, U.value_ids()[1])) == sorted(map(order_key, live + low))


def test_key_collision_check_still_fires_after_a_key_sweep(monkeypatch):
    U = Universe()
    monkeypatch.setattr(interning, "key_id", lambda t: 42 if isinstance(t, str) else interning.splitmix64(t))
    assert U.key("a") == 42
    with pytest.raises(RuntimeError, match="collision"):
        U.key("b")
    U.key(1)
    U.key(2)
    flags = np.array([kid == 42 or kid == interning.splitmix64(1) for kid in U.key_ids().tolist()], np.uint8)
    assert U.sweep(np.zeros(0, np.uint8), flags)["keys"] == (3, 2)
    with pytest.raises(RuntimeError, match="collision"):  # "a" survived: its id is still taken
        U.key("b")
    assert U.key("a") == 42
    U.sweep(np.zeros(0, np.uint8), np.zeros(2, np.uint8))
    assert U.key("b") == 42  # "a" is gone: the id is free, and may name another term now
    with pytest.raises(RuntimeError, match="collision"):
        U.key("a")


def test_snapshot_written_after_a_sweep_restores_the_swept_tables(tmp_path):
    U = Universe()
    terms = _terms(60)
    vids = [U.value(t) for t in terms]
    keys = [f"key{i}" for i in range(8)]
    kids = [U.key(k) for k in keys]
    U.node(Atom("n1"))
    live_i = [i for i in range(len(terms)) if i % 4 == 0][:8]
    U.key("unused")  # no row names it
    kflags = np.isin(U.key_ids(), np.array(kids, np.uint64))
    U.sweep(_flags(U, [terms[i] for i in live_i]), kflags)
    rows = (np.array(kids, np.uint64), np.array([vids[i] for i in live_i], np.uint64),
            np.arange(8, dtype=np.int64), np.zeros(8, np.uint32), np.arange(1, 9, dtype=np.uint64))
    order = np.argsort(rows[0])
    rows = tuple(c[order] for c in rows)
    path = str(tmp_path / "snap")
    storage.write_arrays(path, Atom("n1"), 3, rows, (0, np.zeros(1, np.uint32), np.array([8], np.uint64)), U)
    _node, _seq, rows2, _ctx, U2, _m = storage.read_arrays(path)
    assert U2.value_ids()[0] == U.value_ids()[0]
    assert [order_key(t) for t in U2.value_ids()[1]] == [order_key(t) for t in U.value_ids()[1]]
    assert U2.value_count() == 8 and U2.key_count() == 8
    assert U2.key_ids().tolist() == U.key_ids().tolist()
    for a, b in zip(U2.term_tables(), U.term_tables()):
        assert np.array_equal(a, b)
    for v in rows2[1].tolist():
        assert order_key(U2.value_term(v)) == order_key(U.value_term(v))
    with pytest.raises(KeyError):
        U2.value_term(vids[1])
