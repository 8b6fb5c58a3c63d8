"""Host mirror of the data path of `DeltaCrdt.CausalCrdt` around the join (reference
lib/delta_crdt/causal_crdt.ex): applying a delta to a replica's state and the diffs
its `on_diffs` subscriber receives.  The GenServer, neighbours and sync messages are
out of scope here (tests/binding_mirror.py restates the handlers over the NIF's
mirror).  The MerkleMap (aw_lww_map.merkle_map, store.MerkleTree) and the
sharded round (sharding.py, §6) are in scope and have modules of their own.  So has storage
(storage.py): the whole-state snapshot the reference's write_to_storage would write after
every delta (causal_crdt.ex:238-250), and beside it the per-delta journal
(§4.18) that the two resident update functions below append to when given one -- the part
of update_state_with_delta's write_to_storage (:383-404) a resident replica can afford.

    from delta_crdt_ex_amd import aw_lww_map as M, causal_crdt as CC
    st = M.compress_dots(M.new())
    st, diffs = CC.update_state_with_delta(st, M.add("k", "v", 1, st), ["k"])
    diffs                                   # => [("add", "k", "v")]

update_state_with_delta/3 (:383-404) runs join/3 and diff/3 (:343-351) as ONE
libdeltagpu call (dg_join2_changes: the changed keys come out of the join's merge),
then diffs_to_callback/3 (:359-381) reads the changed keys on the old and on the new
state in one more (dg_read_diff) and keeps the keys whose read value changed.

update_resident_state_with_delta does the same to a state that stays on the device and
is joined in place (dg_join_delta_home_diffs for a mutation or a small sync delta, else
dg_join_delta_diffs: the join, the changed keys, the MerkleMap update and both reads in one
call) -- the old rows are overwritten, so the reads before the join come out of the join
itself.  update_resident_state_with_deltas takes a batch of pending deltas in one call
(dg_join_deltas): the one-pass fold, then the streaming diff of the state before and after.
"""
from __future__ import annotations

import numpy as np
import torch

from . import aw_lww_map as M
from ._abi import DG_DIFF_NEW, DG_DIFF_OLD
from .store import Context, Store, u64


HOME_KEYS, HOME_ROWS, HOME_CTX = 512, 512, 1024  # dg_join_delta_home's limits on the delta


def _keyset(U, keys):
    """`keys` as (key id, key) pairs in the caller's order, and the ascending unique ids on
    the device (keys by interned id, not Python equality)."""
    order = [(U.key(k), k) for k in keys]
    kids = np.array(sorted({kid for kid, _ in order}), dtype=np.uint64)
    return order, torch.from_numpy(np.ascontiguousarray(kids).view(np.int64)).to(M._dev())


def _callback_diffs(U, order, changed, old_val, new_val, flags):
    """diffs_to_callback/3 (:361-381) from the device's reads of the changed keys (numpy
    arrays): a list of ("add", key, value) / ("remove", key) in `keys` order."""
    by = {int(k): (int(f), int(o), int(n)) for k, o, n, f in zip(changed, old_val, new_val, flags)}
    diffs = []
    for kid, k in order:
        if kid not in by:
            continue
        f, o, n = by[kid]
        # Map.get(read, key) (:369): nil for an absent key AND for a key whose value is nil
        o = o if f & DG_DIFF_OLD and U.value_term(o) is not None else None
        n = n if f & DG_DIFF_NEW and U.value_term(n) is not None else None
        if o == n:  # {old, old} -> []  (value ids: equal exactly when the terms are =:=)
            continue
        # {_old, nil} -> {:remove, key}  (delta_subscriber_test.exs:26-27); else {:add, ...}
        diffs.append(("remove", k) if n is None else ("add", k, U.value_term(n)))
    return diffs


def _make_room(state: M.AWLWWMap, spare: Store, n_ctx: int, n_rows: int):
    """Room in the resident state's context for `n_ctx` more entries and in `spare` for the
    state's rows plus `n_rows`: both grow by doubling what the join needs."""
    rows, ctx = state.rows, state.ctx
    need = ctx.n + n_ctx
    if ctx.cap < need:  # room for the union (a resident replica's context grows by doubling)
        grown = Context.empty(ctx.kind, 2 * need, rows.device)
        grown.node[: ctx.n].copy_(ctx.node[: ctx.n])
        grown.cnt[: ctx.n].copy_(ctx.cnt[: ctx.n])
        ctx.node, ctx.cnt = grown.node, grown.cnt
    if spare.cap < rows.n + n_rows:  # (the spare holds no rows: nothing to copy)
        spare.swap_columns(Store.empty(2 * (rows.n + n_rows), rows.device))


def update_state_with_delta(state: M.AWLWWMap, delta: M.AWLWWMap, keys):
    """Returns (new_state, diffs): diffs is what on_diffs would receive -- None when no
    key's value map changed (diffs_to_callback/3 is not reached), else a list of
    ("add", key, value) / ("remove", key) in `keys` order (possibly empty).  A key listed
    twice is reported twice, as diff/3's and diffs_to_callback/3's flat_map over `keys`
    does (:345,368); values compare exactly (`=:=`: 1, 1.0 and true stay distinct), as
    the reference's map lookups and `{old, old}` match do, and a nil value reads as an
    absent key (H9)."""
    U = state.universe
    order, kt = _keyset(U, keys)
    eng = M.engine()
    out, octx, changed = eng.join2_changes(state.rows, state.ctx, delta.rows, delta.ctx, keys=kt)
    new = M.AWLWWMap(out, octx, U)
    if changed.numel() == 0:
        return new, None
    old_val, new_val, flags = eng.read_diff(state.rows, out, changed)
    return new, _callback_diffs(U, order, u64(changed), u64(old_val), u64(new_val), flags.cpu().numpy())


def _changed_rows_out(n_keys: int, n_delta_rows: int, device) -> Store:
    """Room for a join's changed keys' rows (dg_join_delta_rows' `rows`): a few per key."""
    return Store.empty(4 * n_keys + n_delta_rows + 16, device)


def _journal_effect(journal, state: M.AWLWWMap, tree, changed, rows, ctx=None):
    """Append the effect of the delta(s) just joined: `changed` (ascending key ids, numpy) and
    their joined `rows` -- five numpy columns, or the Store the join filled; where the join
    reports more rows than the Store holds (rows.n > rows.cap: not written, deltagpu.h) they
    are taken from the joined state instead -- with the joined context (`ctx` = (node, cnt)
    when the join brought it home) and the tree's root behind it."""
    if isinstance(rows, Store):
        if rows.n > rows.cap:
            kt = torch.from_numpy(np.ascontiguousarray(changed).view(np.int64).copy()).to(state.rows.device)
            rows = M.engine().take_keys(state.rows, kt)
        rows = rows.to_numpy()
    node, cnt = ctx if ctx is not None else state.ctx.to_numpy()
    journal.append(journal.sequence_number + 1, changed, rows, (state.ctx.kind, node, cnt),
                   root=tree.root() if tree is not None else None)


def update_resident_state_with_delta(state: M.AWLWWMap, delta: M.AWLWWMap, keys, spare: Store,
                                     tree=None, journal=None):
    """update_state_with_delta on a state that stays resident: `state` itself becomes the
    join (its rows in place, or through `spare` when a key's row count changed; its context
    the union; `tree`, a MerkleTree over its rows, follows) and the same `diffs` value is
    returned.  Nothing of the old state is kept on the host or read back: the reads before
    the join come out of the join's own walk of each key (Engine.join_delta_diffs).

    `journal` (a storage.Journal for this replica's base): one record is appended per call --
    the changed keys and their joined rows, which the join brings home anyway, with the joined
    context, sequence number journal.sequence_number + 1 and the tree's root (a call that
    changes no key still records the context).  The journal is for the deltas CausalCrdt
    makes, whose rows all lie in their keyset: for those the join's `changed` is exact
    (deltagpu.h, dg_join_delta), and so the record is the whole effect.  A delta with rows
    outside its keyset changes keys `changed` does not name; the root in the record is what
    catches that, when storage.read replays the journal and compares."""
    U = state.universe
    order, kt = _keyset(U, keys)
    eng = M.engine()
    rows, ctx = state.rows, state.ctx
    _make_room(state, spare, delta.ctx.n, delta.rows.n)
    home = None
    if kt.numel() <= HOME_KEYS and delta.rows.n <= HOME_ROWS and delta.ctx.n <= HOME_CTX:
        # a mutation or a small sync delta: the one-launch join gives the diffs too
        # (dg_join_delta_home_diffs); None: over its other limits, nothing happened
        home = eng.join_delta_home_diffs(rows, ctx, delta.rows, delta.ctx, kt, spare, tree)
    state._host = None
    if home is not None:
        changed, (old_val, new_val, flags) = home[0], home[4]
        if journal is not None:  # (the home block holds the rows and the context too)
            _journal_effect(journal, state, tree, changed, home[1], home[2])
    else:
        out = _changed_rows_out(int(kt.numel()), delta.rows.n, rows.device) if journal is not None else None
        changed, old_val, new_val, flags, _ = eng.join_delta_diffs(rows, ctx, delta.rows, delta.ctx, kt,
                                                                   spare, tree, rows=out)
        changed, old_val, new_val, flags = u64(changed), u64(old_val), u64(new_val), flags.cpu().numpy()
        if journal is not None:
            _journal_effect(journal, state, tree, changed, out)
    if len(changed) == 0:
        return None
    return _callback_diffs(U, order, changed, old_val, new_val, flags)


def update_resident_state_with_deltas(state: M.AWLWWMap, batch, spare: Store, tree=None, journal=None):
    """update_resident_state_with_delta for a batch [(delta, keys), ...] -- the pending
    {:diff, delta, keys} messages of a replica's mailbox -- as ONE call (Engine.join_deltas_keyed, or
    Engine.join_deltas for a batch that declines: the fold, the changed keys, the MerkleMap
    step and both reads; the keyed attempt is made whatever the state's size, see below).  `state` becomes the fold
    of the joins through `spare`, and the same `diffs` value is returned, NET over the batch:
    a key is reported once, with its read before the first and after the last delta (a key
    whose read went a -> b -> a reports nothing; the per-delta callbacks the reference would
    have made are not reproduced), in the order of each key's first occurrence over the
    batch's key lists.  A batch of one delta is the single-delta function.  `journal`: as for
    the single-delta function, ONE record for the batch -- its net changed keys and their rows
    after the last delta."""
    batch = list(batch)
    if len(batch) == 1:
        return update_resident_state_with_delta(state, batch[0][0], batch[0][1], spare, tree, journal)
    U = state.universe
    eng = M.engine()
    order, seen, kts = [], set(), []
    for _, keys in batch:
        o, kt = _keyset(U, keys)
        kts.append(kt)
        for kid, k in o:
            if kid not in seen:
                seen.add(kid)
                order.append((kid, k))
    if not batch:
        return None
    rows, ctx = state.rows, state.ctx
    _make_room(state, spare, sum(d.ctx.n for d, _ in batch), sum(d.rows.n for d, _ in batch))
    state._host = None
    args = (rows, ctx, [d.rows for d, _ in batch], [d.ctx for d, _ in batch], kts, spare, tree)
    # the fold per key of the keysets' union where the library serves the batch (VV contexts,
    # every delta row's key in its keyset), else the streaming fold: the same results.  This
    # mirror always tries the keyed call: on a state of about a million keys that is slower
    # than the streaming fold alone at every batch size measured, and a batch
    # declined on the device has paid for the attempt before the streaming fold runs.
    out = None
    if journal is not None:
        out = _changed_rows_out(sum(int(kt.numel()) for kt in kts), sum(d.rows.n for d, _ in batch), rows.device)
    got = eng.join_deltas_keyed(*args, rows=out)
    changed, old_val, new_val, flags, _ = got if got is not None else eng.join_deltas(*args, rows=out)
    if journal is not None:
        _journal_effect(journal, state, tree, u64(changed), out)
    if changed.numel() == 0:
        return None
    return _callback_diffs(U, order, u64(changed), u64(old_val), u64(new_val), flags.cpu().numpy())


def apply_ops(state: M.AWLWWMap, ops, node_id):
    """A batch of mutate/3 calls (causal_crdt.ex:337-342 per op) applied as ONE delta:
    (new_state, diffs) as update_state_with_delta/3 would give for the batch's touched
    keys (on_diffs sees the batch's net changes, not each op's)."""
    delta, keys = M.mutate_batch(ops, node_id, state)
    return update_state_with_delta(state, delta, keys)


def update_resident_state_with_ops(state: M.AWLWWMap, ops, node_id, spare: Store, tree=None, journal=None):
    """apply_ops on a state that stays resident: the ops (M.mutate_batch's) are applied to
    `state` itself as update_resident_state_with_delta applies their delta, and the same
    `diffs` value is returned -- over the touched keys in ascending key-id order, as apply_ops
    lists them -- with the same journal record.  A batch of at most 512 ops goes down as ONE
    launch and wait (Engine.mutate_home_diffs: the delta is built and joined on the device and
    its dot list never made); a batch the library declines has touched nothing and takes
    M.mutate_batch and update_resident_state_with_delta."""
    U = state.universe
    nid, arrays, n_adds = M.marshal_ops(ops, node_id, state)
    eng = M.engine()
    home = None
    if len(ops) <= HOME_KEYS:
        _make_room(state, spare, 1, len(ops))
        home = eng.mutate_home_diffs(state.rows, state.ctx, nid, *arrays, n_adds, spare, tree)
    if home is None:
        delta, dots, keys = eng.mutate_batch(state.rows, state.ctx, nid, *arrays, n_adds)
        return update_resident_state_with_delta(state, M.AWLWWMap(delta, dots, U),
                                                [U.key_term(int(k)) for k in u64(keys)], spare, tree, journal)
    state._host = None
    changed, (old_val, new_val, flags) = home[0], home[4]
    if journal is not None:
        _journal_effect(journal, state, tree, changed, home[1], home[2])
    if len(changed) == 0:
        return None
    order = [(int(k), U.key_term(int(k))) for k in np.unique(u64(arrays[1]))]
    return _callback_diffs(U, order, changed, old_val, new_val, flags)


__all__ = ["update_state_with_delta", "update_resident_state_with_delta",
           "update_resident_state_with_deltas", "apply_ops", "update_resident_state_with_ops"]
