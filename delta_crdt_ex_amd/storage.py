"""SoA snapshots of a replica's state: what `DeltaCrdt.Storage`
persists -- `{node_id, sequence_number, crdt_state, merkle_map}` (reference
lib/delta_crdt/storage.ex:12-16, written by causal_crdt.ex:238-250 after every delta
and read back at start-up by :216-234) -- stored as the device-resident dot store
itself instead of the term tree.

    storage.write(path, node_id, sequence_number, state, tree)   # AWLWWMap mirror state
    node_id, sequence_number, state, tree = storage.read(path)

File layout (little-endian), one self-describing file per replica:

    b"DGSNAP02" | u64 header length | header (msgpack) | column bytes ...

The header holds node_id, sequence_number, the row and context counts, the context
kind, the byte length and xxh64 of each column, and the exact interning tables of
the state's Universe (keys, values and nodes as tagged terms), so `read` restores the
same terms, ids and rows.  Columns are the raw SoA arrays (key, val, ts, node, cnt,
ctx node, ctx cnt, and the Merkle tree's nodes and per-bucket row counts when one is
persisted; the header records whether the tree hashed terms or ids): 36 B per dot + 12 B per context entry + 8 B per tree node + 2 B per bucket,
copied device -> host by one D2H copy each.  A persisted tree hashes terms (the
Universe's term hashes, interning.py), so it is valid for the restored ids.  The header names the tree's depth and key-hash shard.  A checksum mismatch
raises; the file is written to a temporary name, fsynced and renamed over the old one.

A snapshot is the whole state, so it is written rarely.  What is written per applied delta is
one record of the journal beside it, `<path>.journal` (format and crash cases below, at
`Journal`): the delta's changed keys and their rows, which the join brings
home anyway.

    j = storage.checkpoint(path, node_id, sequence_number, state, tree)   # write + fresh journal
    causal_crdt.update_resident_state_with_delta(state, delta, keys, spare, tree, journal=j)
    node_id, sequence_number, state, tree = storage.read(path)   # base, then ONE dg_replace_keysets

`read_arrays` does the same on the host (`replay_arrays`: the last record naming a key wins).
With no journal file both read exactly what they read before there was one.
"""
from __future__ import annotations

import os
import struct

import msgpack
import numpy as np
import xxhash

from . import interning
from .terms import Atom, EList, EMap

MAGIC = b"DGSNAP02"
# DGSNAP01 (round 2): [id, term] node pairs and one value-id region; its ids do not carry
# over to the closed-form integer ids of DGSNAP02, so such a file is refused, not guessed.
_OLD_MAGICS = (b"DGSNAP01",)
_COLS = (("key", np.uint64), ("val", np.uint64), ("ts", np.int64), ("node", np.uint32),
         ("cnt", np.uint64))


def _pack(t):
    """A term as a tagged msgpack-able value (exact: no pickling)."""
    if t is None:
        return ["n"]
    if isinstance(t, bool):
        return ["b", t]
    if isinstance(t, Atom):
        return ["a", str(t)]
    if isinstance(t, int):
        return ["i", str(t)]
    if isinstance(t, float):
        return ["f", t]
    if isinstance(t, EList):
        return ["l", [_pack(x) for x in t]]
    if isinstance(t, EMap):
        return ["m", [[_pack(k), _pack(v)] for k, v in t]]
    if isinstance(t, tuple):
        return ["t", [_pack(x) for x in t]]
    if isinstance(t, str):
        return ["s", t]
    if isinstance(t, bytes):
        return ["y", t]
    raise TypeError(f"cannot snapshot term {t!r}")


def _unpack(x):
    tag = x[0]
    if tag == "n":
        return None
    if tag == "b":
        return bool(x[1])
    if tag == "a":
        return Atom(x[1])
    if tag == "i":
        return int(x[1])
    if tag == "f":
        return float(x[1])
    if tag == "l":
        return EList(_unpack(v) for v in x[1])
    if tag == "m":
        return EMap((_unpack(k), _unpack(v)) for k, v in x[1])
    if tag == "t":
        return tuple(_unpack(v) for v in x[1])
    if tag == "s":
        return x[1]
    if tag == "y":
        return bytes(x[1])
    raise ValueError(f"bad term tag {tag!r}")


def _universe_tables(U: interning.Universe):
    ids, terms = U.value_ids()
    return {
        "keys": [[str(k), _pack(t)] for k, t in U._key_term.items()],
        "vals": [[str(v), _pack(t)] for v, t in zip(ids, terms)],   # table values, ascending ids
        "nodes": [_pack(t) for t in U._node_term],                  # dense ids 0..n-1
        "val_epoch": U.val_epoch,
    }


def _universe_from(tables) -> interning.Universe:
    U = interning.Universe()
    for k, t in tables["keys"]:
        term = _unpack(t)
        U._key_term[int(k)] = term
        U._key_id[interning._hkey(term)] = int(k)
    for v, t in tables["vals"]:  # ascending ids = term order: appends keep the lists sorted
        term = _unpack(t)
        hk = interning._hkey(term)
        U._val_term[int(v)] = term
        U._val_id[hk] = int(v)
        U._val_keys.append(hk)
        U._val_ids.append(int(v))
        U._val_hash.append(interning.term_hash(term, interning.VAL_SEED))
    for t in tables["nodes"]:
        U.node(_unpack(t))
    U.val_epoch = int(tables.get("val_epoch", 0))
    return U


def write_arrays(path, node_id, sequence_number: int, rows, ctx, universe, merkle=None) -> None:
    """The snapshot file from host arrays: rows = (key, val, ts, node, cnt) numpy columns,
    ctx = (kind, node, cnt), merkle = None or (depth, shard_bits, shard, nodes uint64,
    counts uint16[, terms]) -- `terms` (default True): the tree hashed the rows' terms
    (the Universe's term hashes) rather than their ids; the reader restores it so."""
    cols = [np.ascontiguousarray(c, dt) for c, (_, dt) in zip(rows, _COLS)]
    cols += [np.ascontiguousarray(ctx[1], np.uint32), np.ascontiguousarray(ctx[2], np.uint64)]
    if merkle is not None:
        cols.append(np.ascontiguousarray(merkle[3], np.uint64))
        cols.append(np.ascontiguousarray(merkle[4], np.uint16))
    blobs = [c.tobytes() for c in cols]
    header = {
        "node_id": _pack(node_id),
        "sequence_number": int(sequence_number),
        "rows": int(len(cols[0])),
        "ctx_kind": int(ctx[0]),
        "ctx_n": int(len(cols[5])),
        "merkle": None if merkle is None else [int(merkle[0]), int(merkle[1]), str(int(merkle[2])),
                                               bool(merkle[5]) if len(merkle) > 5 else True],
        "columns": [[len(b), xxhash.xxh64_intdigest(b)] for b in blobs],
        "universe": _universe_tables(universe),
    }
    h = msgpack.packb(header, use_bin_type=True)
    # write-then-rename: a crash mid-write leaves the previous snapshot intact
    tmp = f"{path}.tmp"
    with open(tmp, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<Q", len(h)))
        f.write(h)
        for b in blobs:
            f.write(b)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _read_base(path):
    """read_arrays of the base file alone, and the base's digest and val_epoch."""
    with open(path, "rb") as f:
        magic = f.read(8)
        if magic in _OLD_MAGICS:
            raise ValueError(f"{path}: a {magic.decode()} snapshot (an older layout whose value "
                             f"ids {MAGIC.decode()} does not read); re-create it")
        if magic != MAGIC:
            raise ValueError(f"{path}: not a deltagpu snapshot")
        hl_bytes = f.read(8)
        (hl,) = struct.unpack("<Q", hl_bytes)
        hb = f.read(hl)
        digest = xxhash.xxh64_intdigest(magic + hl_bytes + hb)
        header = msgpack.unpackb(hb, raw=False, strict_map_key=False)
        arrays = []
        dtypes = [d for _, d in _COLS] + [np.uint32, np.uint64, np.uint64, np.uint16]
        for (nbytes, cksum), dt in zip(header["columns"], dtypes):
            b = f.read(nbytes)
            if len(b) != nbytes or xxhash.xxh64_intdigest(b) != cksum:
                raise ValueError(f"{path}: column checksum mismatch")
            arrays.append(np.frombuffer(b, dtype=dt).copy())
    m = header.get("merkle")
    # the 4th entry: term-hashed tree (files without it hold term-hashed trees)
    merkle = None if m is None else (int(m[0]), int(m[1]), int(m[2]), arrays[7], arrays[8],
                                     bool(m[3]) if len(m) > 3 else True)
    got = (_unpack(header["node_id"]), header["sequence_number"], tuple(arrays[:5]),
           (header["ctx_kind"], arrays[5], arrays[6]), _universe_from(header["universe"]), merkle)
    return got, digest


def read_arrays(path):
    """(node_id, sequence_number, rows, ctx, universe, merkle) from a snapshot file as
    host arrays (merkle: None or (depth, shard_bits, shard, nodes, counts, terms)); None if
    absent.  With a journal beside the file whose digest names this base, the records are
    replayed on the host (`replay_arrays`): rows, context, sequence number and the Universe's
    terms are then the state after the last intact record, and the merkle entry keeps the
    tree's shape with nodes and counts None (the base's no longer describe the rows)."""
    if not os.path.exists(path):
        return None
    (node_id, seq, rows, ctx, U, merkle), digest = _read_base(path)
    records = _journal_records(path, digest)
    if not records:
        return node_id, seq, rows, ctx, U, merkle
    for r in records:
        _apply_terms(U, r["terms"])
    last = records[-1]
    if merkle is not None:
        merkle = merkle[:3] + (None, None) + merkle[5:]
    return node_id, last["sequence_number"], replay_arrays(rows, records), last["ctx"], U, merkle


def write(path, node_id, sequence_number: int, state, merkle_map=None) -> None:
    """Storage.write/2's payload {node_id, sequence_number, crdt_state, merkle_map}
    (causal_crdt.ex:242-250) for an AWLWWMap mirror state and its device MerkleTree
    (store.MerkleTree; None: not persisted, rebuilt on read)."""
    m = None
    if merkle_map is not None:
        m = (merkle_map.depth, merkle_map.shard_bits, merkle_map.shard,
             merkle_map.nodes.cpu().numpy().view(np.uint64), merkle_map.bucket_counts(),
             merkle_map.terms is not None)
    write_arrays(path, node_id, sequence_number, state.rows.to_numpy(),
                 (state.ctx.kind,) + tuple(state.ctx.to_numpy()), state.universe, m)


def read(path, device=None):
    """Storage.read/1 (causal_crdt.ex:220-230): {node_id, sequence_number, crdt_state,
    merkle_map} or None if `path` is absent.  The merkle_map is the persisted device tree
    (indexing the restored rows), or None when none was persisted.  With a journal beside the
    file that names this base, its records are applied to the loaded base in ONE
    dg_replace_keysets (the tree follows), the last record's context and sequence number are
    installed, and its root -- when it carries one and a tree was persisted -- must be the
    replayed tree's (ValueError otherwise)."""
    import torch

    from . import aw_lww_map as M
    from .store import Context, MerkleTree, Store, TermHashes
    if not os.path.exists(path):
        return None
    (node_id, seq, rows, ctx, U, merkle), digest = _read_base(path)
    records = _journal_records(path, digest)
    for r in records:  # before the tree hashes a term of theirs
        _apply_terms(U, r["terms"])
    dev = device or M._dev()
    st = Store.from_numpy(*rows, device=dev)
    state = M.AWLWWMap(st, Context.from_numpy(ctx[0], ctx[1], ctx[2], dev), U)
    if merkle is None:
        tree = None
    else:
        depth, sb, shard, nodes, counts, terms = merkle
        # a tree over ids stays one: mixing term-hashed buckets into it after
        # the next update would leave its nodes matching neither kind of rebuild
        tree = MerkleTree.empty(depth, dev, sb, shard, TermHashes.of(U, dev) if terms else None)
        tree.nodes.copy_(torch.from_numpy(nodes.view(np.int64).copy()))
        tree.counts[: 1 << depth].copy_(torch.from_numpy(counts.view(np.int16).copy()))
        tree.store = st
        tree.starts = None  # the chunk index is not persisted: the diff searches until a build
        tree.n_keys = int(len(np.unique(rows[0])))
    if records:
        # the journal: ONE dg_replace_keysets over all records, then the last record's context
        # and sequence number; its root, when it carries one, checks the whole restore
        eng = M.engine()
        key_off = np.concatenate([[0], np.cumsum([len(r["keys"]) for r in records])]).astype(np.int64)
        row_off = np.concatenate([[0], np.cumsum([len(r["rows"][0]) for r in records])]).astype(np.int64)
        kcat = np.concatenate([r["keys"] for r in records] + [np.zeros(1, np.uint64)])  # (never empty)
        keys_cat = torch.from_numpy(kcat.view(np.int64)).to(dev)
        rows_cat = Store.from_numpy(*[np.concatenate([r["rows"][i] for r in records]) for i in range(5)],
                                    device=dev)
        spare = Store.empty(st.n + int(row_off[-1]), dev)
        eng.replace_keysets_cat(st, keys_cat, key_off, rows_cat, row_off, spare, tree)
        last = records[-1]
        seq = last["sequence_number"]
        state.ctx = Context.from_numpy(last["ctx"][0], last["ctx"][1], last["ctx"][2], dev)
        if last["root"] is not None and tree is not None and tree.root() != last["root"]:
            raise ValueError(f"{path}: the replayed tree's root {tree.root():#x} is not the last "
                             f"journal record's {last['root']:#x} (a record is missing or the "
                             "journal was written for other deltas than it holds)")
    return node_id, seq, state, tree


# ---------------------------------------------------------------- the journal
# <path>.journal, beside the snapshot file (the base):
#
#     b"DGJRNL01" | u64 base_digest | record | record | ...
#     record = u64 length | payload | u64 xxh64(payload)
#     payload = u64 sequence_number | u64 root | u32 has_root | u32 ctx_kind
#             | u64 n_ctx | u64 n_keys | u64 n_rows | u64 term bytes
#             | ctx node u32[n_ctx] | ctx cnt u64[n_ctx] | keys u64[n_keys]
#             | key u64[n_rows] | val u64[] | ts i64[] | node u32[] | cnt u64[]
#             | term block (msgpack; empty when the record interned nothing)
#
# base_digest is the xxh64 of the base's magic, header length and msgpack header: the header
# holds every column's checksum, so the digest names the base's content.  A record is the
# EFFECT of one applied delta: the keys it changed, ascending, and those keys' rows after it.
# Replay is "the last record naming a key wins" (replay_arrays; on the device one
# dg_replace_keysets), whatever the CRDT's rules.  The first torn or mismatching record ends
# the journal: what lies before it counts, nothing behind it does.
JOURNAL_MAGIC = b"DGJRNL01"
JOURNAL_HEADER_BYTES = 16
_REC = struct.Struct("<QQIIQQQQ")
RECORD_FIXED_BYTES = 8 + _REC.size + 8  # length | the payload's fixed part | checksum


def journal_path(path) -> str:
    return f"{path}.journal"


def _new_terms(keys, vals, nodes) -> bytes:
    """A record's term block: the terms interned since the base and the earlier records, in
    `_universe_tables`' tagged form (keys [[id, term]], vals [[id, term]], nodes [term])."""
    if not keys and not vals and not nodes:
        return b""
    return msgpack.packb({"keys": [[str(k), _pack(t)] for k, t in keys],
                          "vals": [[str(v), _pack(t)] for v, t in vals],
                          "nodes": [_pack(t) for t in nodes]}, use_bin_type=True)


def _apply_terms(U: interning.Universe, block) -> None:
    """Intern a record's term block into a Universe restored from the base and the records
    before it (ids as recorded; node ids are dense, so the nodes arrive in id order)."""
    if not block:
        return
    import bisect
    for k, t in block["keys"]:
        term = _unpack(t)
        U._key_term[int(k)] = term
        U._key_id[interning._hkey(term)] = int(k)
    for v, t in block["vals"]:
        term = _unpack(t)
        hk = interning._hkey(term)
        if hk in U._val_id:
            continue
        p = bisect.bisect_left(U._val_keys, hk)
        U._val_keys.insert(p, hk)
        U._val_ids.insert(p, int(v))
        U._val_hash.insert(p, interning.term_hash(term, interning.VAL_SEED))
        U._val_id[hk] = int(v)
        U._val_term[int(v)] = term
        U.terms_version += 1
    for t in block["nodes"]:
        U.node(_unpack(t))


def _encode_record(sequence_number, keys, rows, ctx, root, term_block: bytes) -> bytes:
    keys = np.ascontiguousarray(keys, np.uint64)
    cols = [np.ascontiguousarray(c, dt) for c, (_, dt) in zip(rows, _COLS)]
    cn, cc = np.ascontiguousarray(ctx[1], np.uint32), np.ascontiguousarray(ctx[2], np.uint64)
    if len(keys) > 1 and not bool(np.all(keys[1:] > keys[:-1])):
        raise ValueError("journal record: the changed keys must be strictly ascending")
    if len({len(c) for c in cols}) != 1 or len(cn) != len(cc):
        raise ValueError("journal record: columns of unequal length")
    payload = b"".join([_REC.pack(int(sequence_number), int(root or 0) & ((1 << 64) - 1), int(root is not None),
                                  int(ctx[0]), len(cn), len(keys), len(cols[0]), len(term_block)),
                        cn.tobytes(), cc.tobytes(), keys.tobytes()] + [c.tobytes() for c in cols] + [term_block])
    return struct.pack("<Q", len(payload)) + payload + struct.pack("<Q", xxhash.xxh64_intdigest(payload))


def _decode_record(payload: bytes):
    """A record from its payload, or None when the payload's own counts do not add up."""
    if len(payload) < _REC.size:
        return None
    seq, root, has_root, kind, n_ctx, n_keys, n_rows, n_terms = _REC.unpack_from(payload)
    if len(payload) != _REC.size + 12 * n_ctx + 8 * n_keys + 36 * n_rows + n_terms:
        return None
    off = _REC.size

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(payload, dtype=dt, count=n, offset=off).copy()
        off += a.nbytes
        return a

    cn, cc, keys = take(np.uint32, n_ctx), take(np.uint64, n_ctx), take(np.uint64, n_keys)
    rows = tuple(take(dt, n_rows) for _, dt in _COLS)
    terms = msgpack.unpackb(payload[off:], raw=False, strict_map_key=False) if n_terms else None
    return {"sequence_number": seq, "root": root if has_root else None, "ctx": (kind, cn, cc),
            "keys": keys, "rows": rows, "terms": terms}


def _scan_journal(jpath):
    """(base_digest, records, end) of a journal file: the intact records from its start and the
    offset behind the last of them; (None, [], 0) when the file is absent or has no header."""
    if not os.path.exists(jpath):
        return None, [], 0
    with open(jpath, "rb") as f:
        data = f.read()
    if len(data) < JOURNAL_HEADER_BYTES or data[:8] != JOURNAL_MAGIC:
        return None, [], 0
    (digest,) = struct.unpack_from("<Q", data, 8)
    records, off = [], JOURNAL_HEADER_BYTES
    while off + 8 <= len(data):
        (n,) = struct.unpack_from("<Q", data, off)
        if n > len(data) - off - 16:  # torn: the length runs past the file
            break
        payload = data[off + 8: off + 8 + n]
        (ck,) = struct.unpack_from("<Q", data, off + 8 + n)
        rec = _decode_record(payload) if xxhash.xxh64_intdigest(payload) == ck else None
        if rec is None:
            break
        records.append(rec)
        off += 16 + n
    return digest, records, off


def _journal_records(path, base_digest):
    """The intact records of the journal beside `path`; none when it is absent or stale (its
    digest names another base: one written before the last `write` or `checkpoint`)."""
    digest, records, _ = _scan_journal(journal_path(path))
    return records if digest == base_digest else []


def read_journal(path):
    """The intact records of `path`'s journal as dicts (sequence_number, root or None, ctx =
    (kind, node, cnt), keys, rows = five columns, terms = the decoded term block or None);
    [] when the base or the journal is absent or the journal is stale."""
    if not os.path.exists(path):
        return []
    with open(path, "rb") as f:
        head = f.read(16)
        hb = f.read(struct.unpack("<Q", head[8:])[0]) if len(head) == 16 else b""
    return _journal_records(path, xxhash.xxh64_intdigest(head + hb))


def replay_arrays(rows, records):
    """The host restatement of the replay: `rows` (five numpy columns in store order) with
    every record applied in order -- for each key of a record's `keys` the rows of that key
    become the record's rows of it (none: the key is removed) -- computed as "the last record
    naming a key wins".  Returns the five columns."""
    rows = tuple(np.asarray(c, dt) for c, (_, dt) in zip(rows, _COLS))
    nk = [len(r["keys"]) for r in records]
    if sum(nk) == 0:
        return rows
    kcat = np.concatenate([r["keys"] for r in records]).astype(np.uint64)
    rec = np.repeat(np.arange(len(records), dtype=np.int64), nk)
    order = np.argsort(kcat, kind="stable")  # equal keys stay in record order
    ks, rs = kcat[order], rec[order]
    last = np.ones(len(ks), bool)
    last[:-1] = ks[1:] != ks[:-1]
    ukeys, winner = ks[last], rs[last]
    keep = ~np.isin(rows[0], ukeys)
    parts = [tuple(c[keep] for c in rows)]
    for j, r in enumerate(records):
        rk = np.asarray(r["rows"][0], np.uint64)
        if len(rk) == 0:
            continue
        pos = np.searchsorted(ukeys, rk)
        if np.any(pos >= len(ukeys)) or np.any(ukeys[np.minimum(pos, len(ukeys) - 1)] != rk) or \
                np.any(~np.isin(rk, r["keys"])):
            raise ValueError(f"journal record {j}: a row whose key is not in the record's keys")
        mine = winner[pos] == j
        parts.append(tuple(np.asarray(c, dt)[mine] for c, (_, dt) in zip(r["rows"], _COLS)))
    cat = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    # keys are disjoint between the parts and each part is in store order: a stable sort on
    # the key alone restores the store order
    o = np.argsort(cat[0], kind="stable")
    return tuple(c[o] for c in cat)


class Journal:
    """The append side of `<path>.journal` for the base at `path`, which must exist.  Opening
    finds the intact records (a stale journal -- another base's digest -- or none: a fresh
    file), truncates a torn tail, and learns which terms the base and the records already
    hold.  One Journal belongs to one base: after `write` or `checkpoint` make a new one
    (checkpoint returns it).

        j = Journal(path, state.universe)
        j.append(sequence_number, changed_keys, their_rows, (kind, node, cnt), root=tree.root())

    A record is 72 B + 8 B per key + 36 B per row + 12 B per context entry + its term block,
    whatever the state's size."""

    def __init__(self, path, universe: interning.Universe):
        self.path, self.jpath, self.universe = path, journal_path(path), universe
        with open(path, "rb") as f:
            head = f.read(16)
            if head[:8] != MAGIC:
                raise ValueError(f"{path}: not a deltagpu snapshot")
            hb = f.read(struct.unpack("<Q", head[8:])[0])
        self.base_digest = xxhash.xxh64_intdigest(head + hb)
        header = msgpack.unpackb(hb, raw=False, strict_map_key=False)
        tables = header["universe"]
        # the last record's sequence number (the base's while there is none)
        self.sequence_number = int(header["sequence_number"])
        self.val_epoch = int(tables.get("val_epoch", 0))
        self._keys = {int(k) for k, _ in tables["keys"]}
        self._vals = {int(v) for v, _ in tables["vals"]}
        self._n_nodes = len(tables["nodes"])
        digest, records, end = _scan_journal(self.jpath)
        if digest != self.base_digest:  # absent or stale: replaced
            records, end = [], JOURNAL_HEADER_BYTES
            with open(self.jpath, "wb") as f:
                f.write(JOURNAL_MAGIC + struct.pack("<Q", self.base_digest))
                f.flush()
                os.fsync(f.fileno())
        for r in records:
            if r["terms"]:
                self._keys.update(int(k) for k, _ in r["terms"]["keys"])
                self._vals.update(int(v) for v, _ in r["terms"]["vals"])
                self._n_nodes += len(r["terms"]["nodes"])
        self.n_records = len(records)
        if records:
            self.sequence_number = int(records[-1]["sequence_number"])
        self._f = open(self.jpath, "r+b")
        self._f.truncate(end)  # a torn tail goes before the first append
        self._f.seek(end)
        # what the Universe looked like when its terms were last compared with the sets above
        self._seen = None

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _term_block(self):
        """(block, written): the terms the Universe holds and the base and earlier records do
        not, and the callback that marks them as held once the record is written.  Keys are
        only ever appended until a sweep, so the new ones are the dict's tail; the value table
        is walked when the term-hash tables moved, the key table only after a sweep."""
        U = self.universe
        seen = (U.terms_version, U.sweeps, len(U._key_term))
        if seen == self._seen:
            return b"", lambda: None
        keys, vals = [], []
        if self._seen is None or U.sweeps != self._seen[1]:
            keys = [(k, t) for k, t in U._key_term.items() if k not in self._keys]
        else:
            for k in reversed(U._key_term):
                if len(keys) == len(U._key_term) - self._seen[2]:
                    break
                if k not in self._keys:
                    keys.append((k, U._key_term[k]))
            keys.reverse()
        if self._seen is None or U.terms_version != self._seen[0]:
            vals = [(v, U._val_term[v]) for v in U._val_ids if v not in self._vals]
        nodes = U._node_term[self._n_nodes:]

        def written():  # (only once the record holding them is in the file)
            self._seen = seen
            self._keys.update(k for k, _ in keys)
            self._vals.update(v for v, _ in vals)
            self._n_nodes += len(nodes)

        return _new_terms(keys, vals, nodes), written

    def append(self, sequence_number, keys, rows, ctx, root=None, fsync=True) -> int:
        """One record: the changed `keys` (ascending uint64), their `rows` after the delta
        (five columns, store order; a key without rows was removed), the state's context
        (kind, node, cnt) and, optionally, the tree's root after it.  Returns the bytes
        written.  fsync=False leaves the flush to disk to a caller that groups commits."""
        if self.universe.val_epoch != self.val_epoch:
            raise ValueError(f"{self.jpath}: the Universe's val_epoch is {self.universe.val_epoch}, the "
                             f"base's {self.val_epoch}: a value remap rewrote ids across the store, "
                             "which no per-key record expresses -- checkpoint instead")
        block, written = self._term_block()
        blob = _encode_record(sequence_number, keys, rows, ctx, root, block)
        self._f.write(blob)
        self._f.flush()
        if fsync:
            os.fsync(self._f.fileno())
        written()
        self.n_records += 1
        self.sequence_number = int(sequence_number)
        return len(blob)


def checkpoint(path, node_id, sequence_number: int, state, merkle_map=None) -> Journal:
    """`write`, then a fresh empty journal: the new base first (temporary file, rename), the
    journal second.  A crash in between leaves the old journal beside the new base; its digest
    names the old base, so it is ignored on read and replaced here or by the next Journal."""
    write(path, node_id, sequence_number, state, merkle_map)
    return Journal(path, state.universe)


__all__ = ["write", "read", "write_arrays", "read_arrays", "MAGIC", "Journal", "checkpoint",
           "replay_arrays", "read_journal", "journal_path", "JOURNAL_MAGIC", "JOURNAL_HEADER_BYTES",
           "RECORD_FIXED_BYTES"]
