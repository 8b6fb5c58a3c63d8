"""k pending get_diff / send_diff messages answered by ONE call on the device-resident
replica, through the NIF's mirror (delta_crdt_ex_amd/nif.py take_batch -> c_src/replica_take.c
dgr_take_batch -> dg_take_keysets): element j equals take(state, version, keysets[j]) and
the term oracle's Map.take, for keysets given unsorted, with duplicates and with keys the state
lacks; more than 64 keysets are chunked; the version does not move; an older version is
refused as take refuses it; a call after a join sees the joined rows; and the union's rows
come home once."""
import ctypes as C
import random

import numpy as np
import pytest

import binding_mirror as B
from delta_crdt_ex_amd import nif
from oracle.erlterm import tg
from test_gpu_replica_diffs import _peer, gpu_node  # noqa: F401 (gpu_node: the fixture)

pytestmark = pytest.mark.gpu

N_KEYS = 2500  # the state's keys are 0 .. N_KEYS - 1, two entries each


@pytest.fixture(scope="module")
def base():
    return _peer([1, 2], list(range(N_KEYS)), lambda j, i: (j, i) if i % 4 else float(i), 100)


def _resident(terms):
    st = B.attach_gpu(terms, 0)
    assert st.gpu is not None
    return st.gpu[0], st.gpu[1]


def _keysets(k, seed):
    """k key lists in no order: a sixth of each outside the state, ten keys twice."""
    rng = random.Random(seed)
    out = []
    for j in range(k):
        ks = [rng.randrange(0, N_KEYS + N_KEYS // 5) for _ in range(150 + 3 * j)]
        ks += ks[:10]
        rng.shuffle(ks)
        out.append([tg(x) for x in ks])
    return out


def _map_take(terms, keys):
    return {k: terms.value[k] for k in set(keys) if k in terms.value}


@pytest.mark.parametrize("k", [3, 70])
def test_take_batch_is_k_takes(base, k):
    res, ver = _resident(base)
    sets = _keysets(k, k)
    assert any(x not in base.value for x in sets[0]) and len(set(sets[0])) < len(sets[0])
    r = nif.take_batch(res, ver, sets)
    assert r[0] == "ok" and len(r[1]) == k
    for j, keys in enumerate(sets):
        single = nif.take(res, ver, keys)
        assert single[0] == "ok" and r[1][j] == single[1] == _map_take(base, keys), j
    assert res.version == ver  # a read: the version does not move on
    assert nif.take_batch(res, ver, []) == ("ok", [])
    assert nif.take_batch(res, ver, [[], [tg(N_KEYS + 7)]]) == ("ok", [{}, {}])


def test_stale_version_and_a_call_after_a_join(base):
    res, ver = _resident(base)
    sets = _keysets(3, 11)
    stale = nif.take(res, ver + 1, sets[0])
    assert stale == ("error", "stale") and nif.take_batch(res, ver + 1, sets) == stale
    # a peer's delta over keys the state holds and keys it lacks
    keys = list(range(N_KEYS - 20, N_KEYS + 20))
    peer = B.detach(_peer([9], keys, lambda j, i: ("new", i), 900))
    tkeys = [tg(x) for x in keys]
    r = nif.join_delta(res, ver, peer.dots, peer.value, tkeys)
    assert r[0] == "ok" and r[1] == ver + 1
    after = B.join_cpu(base, peer, tkeys)
    assert nif.take_batch(res, ver, sets) == ("error", "stale")
    sets.append(tkeys)
    got = nif.take_batch(res, ver + 1, sets)
    assert got[0] == "ok"
    for j, ks in enumerate(sets):
        assert got[1][j] == nif.take(res, ver + 1, ks)[1] == _map_take(after, ks), j
    assert len(got[1][3]) == len(keys) and res.version == ver + 1


def test_the_unions_rows_come_home_once(base):
    """Three identical keysets: the raw dgr_taken holds every row once (rows.n ==
    offs[n_keys], the single take's count), not three times."""
    res, ver = _resident(base)
    eng = res.engine
    kid = nif._marshal_keys(eng, [tg(x) for x in range(0, N_KEYS, 3)])
    single = nif.dg_store()
    assert eng.lib.dgr_take(res.ptr, ver, kid.ctypes.data, len(kid), C.byref(single)) == 0
    n_single = int(single.n)
    # as marshalled, ascending (copied, not sorted by the pack), descending
    rc, tk = nif._take_batch_raw(res, ver, [kid, np.sort(kid), kid[::-1].copy()])
    assert rc == 0
    nu = int(tk.n_keys)
    offs = nif._arr(tk.offs, nu + 1, np.uint64)
    assert nu == len(kid) and np.array_equal(nif._arr(tk.keys, nu, np.uint64), np.sort(kid))
    assert np.all(nif._arr(tk.masks, nu, np.uint64) == 7)
    assert int(tk.rows.n) == int(offs[nu]) == n_single == 2 * len(kid)
