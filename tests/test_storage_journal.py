"""The snapshot journal (delta_crdt_ex_amd/storage.py) on the CPU: the record
format and its size, the crash cases, and the replay's semantics against the C oracle's
keyed joins and a naive per-record replay."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import journal_cases as J
from delta_crdt_ex_amd import interning, storage
from delta_crdt_ex_amd.terms import Atom, EList
from delta_crdt_ex_amd.workloads import VV, vv


def _base(path, rows, ctx, U, seq=5):
    storage.write_arrays(path, Atom("replica"), seq, rows, ctx, U)


def _state(rng, n_keys=40, seed=1):
    keys = J.key_space(n_keys, seed)
    rows, c = J.rows_for(rng, keys, 0, 1)
    return keys, rows, vv({0: c - 1})


def _tables(U):
    t = storage._universe_tables(U)
    return ({k: v for k, v in t["keys"]}, {k: v for k, v in t["vals"]}, t["nodes"], t["val_epoch"])


def _history(tmp_path, n_records=5):
    """A base and `n_records` appended records (one without keys, one removing keys, several
    interning new terms); returns (path, U, rows, ctx, the records as written)."""
    rng = np.random.default_rng(11)
    U = interning.Universe()
    U.key("base key"), U.value("base value"), U.node(Atom("n0"))
    keys, rows, ctx = _state(rng)
    p = tmp_path / "r.dgsnap"
    _base(p, rows, ctx, U)
    j = storage.Journal(p, U)
    written, counter = [], 10_000
    for i in range(n_records):
        if i == 1:  # nothing changed but the context
            ks, rs = np.zeros(0, np.uint64), J.empty_rows()
        else:
            ks = np.sort(rng.choice(keys, 7, replace=False))
            rs, counter = J.rows_for(rng, ks, 1, counter, p_none=0.6 if i == 2 else 0.2)
            U.key(("new key", i)), U.value(EList([i, "v"])), U.node(("node", i))
        cx = vv({0: 100, 1: counter})
        j.append(6 + i, ks, rs, cx, root=0xABC0 + i if i % 2 else None)
        written.append(J.record(ks, rs, 6 + i, cx, 0xABC0 + i if i % 2 else None))
    j.close()
    return p, U, rows, ctx, written


def _same_record(a, b):
    return (a["sequence_number"] == b["sequence_number"] and a["root"] == b["root"]
            and a["ctx"][0] == b["ctx"][0] and np.array_equal(a["ctx"][1], b["ctx"][1])
            and np.array_equal(a["ctx"][2], b["ctx"][2]) and np.array_equal(a["keys"], b["keys"])
            and J.rows_equal(a["rows"], b["rows"]))


def test_record_round_trip(tmp_path):
    p, U, rows, ctx, written = _history(tmp_path)
    got = storage.read_journal(p)
    assert len(got) == len(written) and all(_same_record(a, b) for a, b in zip(got, written))
    assert len(got[1]["keys"]) == 0 and got[1]["terms"] is None  # the zero-key record
    removed = np.setdiff1d(got[2]["keys"], got[2]["rows"][0])
    assert len(removed) > 0  # a record that removes keys
    node_id, seq, r_rows, r_ctx, V, merkle = storage.read_arrays(p)
    assert node_id == Atom("replica") and seq == written[-1]["sequence_number"] and merkle is None
    assert r_ctx[0] == VV and np.array_equal(r_ctx[1], written[-1]["ctx"][1])
    assert np.array_equal(r_ctx[2], written[-1]["ctx"][2])
    assert J.rows_equal(r_rows, J.naive_replay(rows, written))
    # (a later record may add a removed key again: the keys are gone right behind record 2)
    assert not np.isin(removed, storage.replay_arrays(rows, got[:3])[0]).any()
    # the terms interned since the base come back with their ids
    assert _tables(V) == _tables(U)
    assert V.key_term(U.key(("new key", 3))) == ("new key", 3)
    assert V.value(EList([4, "v"])) == U.value(EList([4, "v"])) and V.node(("node", 2)) == U.node(("node", 2))
    assert V.value("later") == U.value("later")  # and the next new value gets the same id


def test_no_journal_reads_as_before(tmp_path):
    rng = np.random.default_rng(2)
    U = interning.Universe()
    keys, rows, ctx = _state(rng)
    p = tmp_path / "r.dgsnap"
    _base(p, rows, ctx, U)
    got = storage.read_arrays(p)
    assert got[1] == 5 and J.rows_equal(got[2], rows) and not os.path.exists(storage.journal_path(p))
    assert storage.read_journal(p) == [] and storage.read_journal(tmp_path / "absent") == []


def test_record_size_is_the_effect_not_the_state(tmp_path):
    """72 B + 8 per key + 36 per row + 12 per context entry + the term block, on a state of
    40 keys and on one of 4000."""
    sizes = []
    for n_keys in (40, 4000):
        rng = np.random.default_rng(3)
        U = interning.Universe()
        keys, rows, ctx = _state(rng, n_keys)
        p = tmp_path / f"r{n_keys}.dgsnap"
        _base(p, rows, ctx, U)
        j = storage.Journal(p, U)
        jp = storage.journal_path(p)
        assert os.path.getsize(jp) == storage.JOURNAL_HEADER_BYTES == 16
        ks = keys[:9]
        rs, _ = J.rows_for(np.random.default_rng(4), ks, 1, 1)
        cx = vv({0: 7, 1: 8, 5: 9})
        n = j.append(6, ks, rs, cx, root=1)
        assert storage.RECORD_FIXED_BYTES == 72
        assert n == 72 + 8 * 9 + 36 * len(rs[0]) + 12 * 3 == os.path.getsize(jp) - 16
        kid, vid, nid = U.key("fresh"), U.value("fresh value"), U.node("fresh node")
        block = storage._new_terms([(kid, "fresh")], [(vid, "fresh value")], ["fresh node"])
        n2 = j.append(7, ks[:0], J.empty_rows(), cx)
        assert n2 == 72 + 12 * 3 + len(block) and os.path.getsize(jp) == 16 + n + n2
        assert j.append(8, ks[:0], J.empty_rows(), cx) == 72 + 12 * 3  # nothing new: no block
        j.close()
        sizes.append((n, n2))
    assert sizes[0] == sizes[1]


def _record_spans(jp):
    data = open(jp, "rb").read()
    spans, off = [], storage.JOURNAL_HEADER_BYTES
    while off < len(data):
        n = int.from_bytes(data[off:off + 8], "little")
        spans.append((off, off + 16 + n))
        off += 16 + n
    return data, spans


def test_truncated_last_record(tmp_path):
    p, U, rows, ctx, written = _history(tmp_path)
    jp = storage.journal_path(p)
    data, spans = _record_spans(jp)
    for cut in (spans[-1][0] + 3, spans[-1][0] + 40, spans[-1][1] - 1):
        open(jp, "wb").write(data[:cut])
        got = storage.read_journal(p)
        assert len(got) == len(written) - 1 and all(_same_record(a, b) for a, b in zip(got, written))
        assert storage.read_arrays(p)[1] == written[-2]["sequence_number"]


@pytest.mark.parametrize("which", ["last", "middle"])
def test_flipped_byte_ends_the_journal(tmp_path, which):
    p, U, rows, ctx, written = _history(tmp_path)
    jp = storage.journal_path(p)
    data, spans = _record_spans(jp)
    i = len(spans) - 1 if which == "last" else 2
    raw = bytearray(data)
    raw[(spans[i][0] + spans[i][1]) // 2] ^= 0x10
    open(jp, "wb").write(bytes(raw))
    got = storage.read_journal(p)
    assert len(got) == i and all(_same_record(a, b) for a, b in zip(got, written))  # none behind it
    assert J.rows_equal(storage.read_arrays(p)[2], J.naive_replay(rows, written[:i]))


def test_append_after_a_torn_tail(tmp_path):
    p, U, rows, ctx, written = _history(tmp_path)
    jp = storage.journal_path(p)
    data, spans = _record_spans(jp)
    open(jp, "wb").write(data[:spans[3][0] + 21])  # record 3 torn, record 4 gone
    j = storage.Journal(p, U)
    assert j.n_records == 3 and j.sequence_number == written[2]["sequence_number"]
    assert os.path.getsize(jp) == spans[3][0]  # truncated there first
    ks = written[0]["keys"][:2]
    j.append(99, ks, J.empty_rows(), written[0]["ctx"])
    j.close()
    got = storage.read_journal(p)
    assert [r["sequence_number"] for r in got] == [6, 7, 8, 99]
    # the terms of the lost records are written again with the next record
    assert _tables(storage.read_arrays(p)[4]) == _tables(U)


def test_stale_journal_is_ignored_and_replaced(tmp_path):
    p, U, rows, ctx, written = _history(tmp_path)
    after = J.naive_replay(rows, written)
    _base(p, after, written[-1]["ctx"], U, seq=50)  # a plain write: the journal names the old base
    assert storage.read_journal(p) == []
    got = storage.read_arrays(p)
    assert got[1] == 50 and J.rows_equal(got[2], after)
    j = storage.Journal(p, U)
    assert j.n_records == 0 and os.path.getsize(storage.journal_path(p)) == 16
    j.append(51, written[0]["keys"], written[0]["rows"], written[0]["ctx"])
    j.close()
    assert [r["sequence_number"] for r in storage.read_journal(p)] == [51]


def test_checkpoint_interrupted_between_its_steps(tmp_path):
    """checkpoint = the new base, then the fresh journal.  A crash in between leaves the old
    journal beside the new base (simulated by putting it back): it is ignored."""
    p, U, rows, ctx, written = _history(tmp_path)
    jp = storage.journal_path(p)
    old_journal = open(jp, "rb").read()
    after = J.naive_replay(rows, written)

    last_ctx = written[-1]["ctx"]
    state = SimpleNamespace(  # what storage.write reads of a mirror state
        rows=SimpleNamespace(to_numpy=lambda: after),
        ctx=SimpleNamespace(kind=VV, to_numpy=lambda: (last_ctx[1], last_ctx[2])), universe=U)
    j = storage.checkpoint(p, Atom("replica"), 60, state)
    assert j.n_records == 0 and j.sequence_number == 60 and os.path.getsize(jp) == 16
    j.close()
    open(jp, "wb").write(old_journal)
    got = storage.read_arrays(p)
    assert got[1] == 60 and J.rows_equal(got[2], after) and storage.read_journal(p) == []


def test_append_refuses_a_changed_val_epoch(tmp_path):
    rng = np.random.default_rng(5)
    U = interning.Universe()
    keys, rows, ctx = _state(rng)
    p = tmp_path / "r.dgsnap"
    _base(p, rows, ctx, U)
    j = storage.Journal(p, U)
    j.append(6, keys[:1], J.empty_rows(), ctx)
    U.value("a"), U.value("b")
    U.relabel()
    size = os.path.getsize(storage.journal_path(p))
    with pytest.raises(ValueError, match="val_epoch.*checkpoint"):
        j.append(7, keys[:1], J.empty_rows(), ctx)
    j.close()
    assert os.path.getsize(storage.journal_path(p)) == size and len(storage.read_journal(p)) == 1


def test_append_refuses_unsorted_keys(tmp_path):
    rng = np.random.default_rng(6)
    U = interning.Universe()
    keys, rows, ctx = _state(rng)
    p = tmp_path / "r.dgsnap"
    _base(p, rows, ctx, U)
    j = storage.Journal(p, U)
    with pytest.raises(ValueError, match="ascending"):
        j.append(6, keys[:3][::-1], J.empty_rows(), ctx)
    j.close()
    assert storage.read_journal(p) == []


def test_replay_of_thirty_keyed_joins(tmp_path):
    """30 keyed joins through the C oracle on a state of 2,000 keys with 1..3 rows each.  After
    each join the changed keys and their rows are derived by comparing the two states, and
    appended; base + journal then read back as the oracle's final state and context, and
    replay_arrays agrees with the record-by-record dict replay."""
    from oracle import ref as R
    rng = np.random.default_rng(30)
    U = interning.Universe()
    keys = J.key_space(2000, 9)
    rows, c0 = J.rows_for(rng, keys, 0, 1)
    ctx = vv({0: c0 - 1})
    base_rows, p = rows, tmp_path / "r.dgsnap"
    _base(p, rows, ctx, U, seq=0)
    j = storage.Journal(p, U)
    counters = {n: 1 for n in (1, 2, 3)}
    n_removed = n_readded = 0
    gone = set()
    for i in range(30):
        node = 1 + i % 3
        ks = np.sort(rng.choice(keys, 120, replace=False))
        # a peer's sync delta: its rows of `ks` (some keys hold none: removed there) under a
        # context that covers every dot of node 0 and of the peer so far
        d_rows, counters[node] = J.rows_for(rng, ks, node, counters[node], p_none=0.3)
        d_ctx = vv({0: c0 - 1, node: counters[node] - 1})
        new_rows, new_ctx = R.join2(rows, ctx, d_rows, d_ctx, ks)
        changed = J.changed_keys(rows, new_rows, ks)
        now_gone = set(changed[~np.isin(changed, new_rows[0])].tolist())
        n_removed += len(now_gone)
        n_readded += len(gone & set(new_rows[0].tolist()))
        gone = (gone | now_gone) - set(new_rows[0].tolist())
        j.append(i + 1, changed, J.take(new_rows, changed), new_ctx)
        rows, ctx = new_rows, new_ctx
    j.close()
    assert n_removed > 50 and n_readded > 5  # removes, and adds after a remove, happened
    node_id, seq, got_rows, got_ctx, V, _ = storage.read_arrays(p)
    assert seq == 30 and J.rows_equal(got_rows, rows)
    assert got_ctx[0] == ctx[0] and np.array_equal(got_ctx[1], ctx[1]) and np.array_equal(got_ctx[2], ctx[2])
    records = storage.read_journal(p)
    assert len(records) == 30
    assert J.rows_equal(storage.replay_arrays(base_rows, records), J.naive_replay(base_rows, records))
    assert max(np.unique(rows[0], return_counts=True)[1]) > 1  # multi-row keys are in play
