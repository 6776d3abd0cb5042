"""epcnet_revisit_search on the device against tests/revisit_ref.py, whose search is the package's own ``knn_search`` called once per distinct
prefix on ``database[:p]`` -- never the entry under test.  Every output goes into a poisoned buffer with guard bytes IN FRONT of it and
behind it, the workspace is exactly the size asked for, and ``dist`` is compared on BIT PATTERNS, ``idx`` and ``count`` exactly: the answer
is the exact k nearest by one definition of the distance, so there is no tolerance anywhere.  Self-searches around the tiles of 64 and 128,
every k against prefixes around k, k + 8 and 64, plateaus, shuffled queries, ties, a set on which the GEMM form cancels, non-finite
descriptors and keys, the whole-call failures, several passes, two runs, one captured graph replayed on other data, the streaming index,
and the engine's descriptors of a small out-and-back drive."""
import numpy as np
import pytest
import torch

import helpers as H
import revisit_ref as R
import submap_ref as SR
from helpers import Guarded, O

pytestmark = pytest.mark.gpu

DIMS = [8, 256]


def _up(a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype))
    if a.size == 0:                                       # an empty tensor has no address: one row stands in and is never read
        a = np.zeros((1,) + a.shape[1:], dtype)
    return torch.from_numpy(a).to("cuda")


def _raw(db, db_along, q, q_along, min_travel, k, pass_queries=0):
    """The entry itself on guarded, poisoned outputs and a guarded workspace of exactly the size asked for -> (dist, idx, count) as numpy."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    nd, nq, dim = len(db), len(q), db.shape[1]
    need = L.lib().epcnet_revisit_workspace_bytes(nd, nq, pass_queries)
    assert need > 0 and need % 16 == 0
    idx, dist, count = Guarded((nq, k), torch.int32, dev), Guarded((nq, k), torch.float32, dev), Guarded((nq,), torch.int32, dev)
    ws = Guarded((need,), torch.uint8, dev)
    L.run.epcnet_revisit_search(_up(db, np.float32), _up(db_along, np.float64), nd, _up(q, np.float32), _up(q_along, np.float64), nq, dim,
                                float(min_travel), k, pass_queries, idx.t, dist.t, count.t, ws.t, need)
    torch.cuda.synchronize()
    for g in (idx, dist, count, ws):
        assert g.intact()
    return dist.t.cpu().numpy(), idx.t.cpu().numpy(), count.t.cpu().numpy()


def _knn(database, queries, k):
    """The oracle's search: the parent's knn_search on device tensors."""
    d, i = H.pkg("retrieval").knn_search(database, queries, k)
    return d.cpu().numpy(), i.cpu().numpy()


def _want(db, db_along, q, q_along, min_travel, k):
    dev_db = torch.from_numpy(np.ascontiguousarray(db, np.float32)).to("cuda")
    dev_q = dev_db if q is db else torch.from_numpy(np.ascontiguousarray(q, np.float32)).to("cuda")
    return R.revisit_reference(_knn, dev_db, db_along, dev_q, q_along, min_travel, k)


def _equal(got, want, what):
    gd, gi, gc = got
    wd, wi, wc = want
    assert gc.tolist() == wc.tolist(), (what, "count")
    bad = np.nonzero((gi != wi).any(1) | (gd.view(np.int32) != wd.view(np.int32)).any(1))[0]
    assert bad.size == 0, (what, "%d rows differ, the first is %d: idx %s / %s, dist %s / %s" % (
        bad.size, bad[0], gi[bad[0]].tolist(), wi[bad[0]].tolist(), gd[bad[0]].tolist(), wd[bad[0]].tolist()))


def _both(db, db_along, q, q_along, min_travel, k, what, pass_queries=0):
    want = _want(db, db_along, q, q_along, min_travel, k)
    got = _raw(db, db_along, q, q_along, min_travel, k, pass_queries)
    _equal(got, want, what)
    return got, want


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 257, 300])
def test_self_search_sizes(T, dim):
    db, along = R.unit_rows(1, T, dim), np.arange(T) * 10.0
    for min_travel in (0.0, 10.0, 25.0, 640.0, 1e9):
        (_, idx, count), _ = _both(db, along, db, along, min_travel, 5, "T %d min_travel %g" % (T, min_travel))
        assert count.tolist() == R.prefix_counts(along, along, min_travel).tolist()
        if min_travel == 0.0:
            assert idx[:, 0].tolist() == list(range(T))                      # the query's own row, at distance 0
        else:
            assert (idx < np.arange(T)[:, None]).all()                       # causal
        if min_travel == 1e9:
            assert (count == 0).all() and (idx == -1).all()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [1, 5, 25, 56])
def test_k_against_prefixes_around_k_and_the_selection_edges(k, dim):
    prefixes = sorted({0, 1, max(k - 1, 0), k, k + 7, k + 8, k + 9, 64, 65})
    db, along = R.unit_rows(2, 80, dim), np.arange(80) * 1.0
    q = R.unit_rows(3, len(prefixes), dim)
    q_along = np.array([100.0 + p - 0.5 for p in prefixes])                  # along <= p - 0.5: the rows 0 .. p - 1
    (dist, idx, count), _ = _both(db, along, q, q_along, 100.0, k, "k %d" % k)
    assert count.tolist() == prefixes
    for row, p in enumerate(prefixes):
        assert (idx[row, :min(k, p)] >= 0).all() and (idx[row, min(k, p):] == -1).all() and np.isinf(dist[row, min(k, p):]).all()


@pytest.mark.parametrize("dim", DIMS)
def test_plateaus_of_equal_along(dim):
    along = np.concatenate([[0.0, 10.0, 20.0], np.full(5, 30.0), [40.0, 50.0], np.full(200, 60.0), [70.0, 80.0, 90.0]])
    db = R.unit_rows(4, len(along), dim)
    for min_travel in (0.0, 10.0):
        (_, _, count), _ = _both(db, along, db, along, min_travel, 5, "plateaus, min_travel %g" % min_travel)
        steps = np.unique(count)
        assert 5 in np.diff(steps) and 200 in np.diff(steps)                 # p jumps by the run length


@pytest.mark.parametrize("dim", DIMS)
def test_shuffled_queries_against_another_database(dim):
    db, along = R.unit_rows(5, 300, dim), np.arange(300) * 10.0
    q = R.unit_rows(6, 300, dim)
    q_along = np.random.default_rng(7).permutation(np.arange(300) * 10.0 + 5.0)
    (_, _, count), _ = _both(db, along, q, q_along, 100.0, 5, "shuffled")
    tile_last = count[127::128]
    assert (count.reshape(-1)[:256].reshape(2, 128).max(1) != tile_last[:2]).all()      # a tile's largest p is not its last query's


@pytest.mark.parametrize("dim", DIMS)
def test_ties_go_to_the_lower_index(dim):
    base = R.unit_rows(8, 40, dim)
    db = np.repeat(base, 3, axis=0)                                          # rows 3 j, 3 j + 1, 3 j + 2 are identical
    along = np.arange(len(db)) * 1.0
    q = np.concatenate([R.unit_rows(9, 20, dim), db[50:51]])                 # the last query IS a database row
    q_along = np.full(len(q), 1000.0)
    (dist, idx, _), _ = _both(db, along, q, q_along, 0.0, 6, "triplicates")
    assert (idx[:, 0] % 3 == 0).all() and (idx[:, 1] == idx[:, 0] + 1).all() and (idx[:, 2] == idx[:, 0] + 2).all()
    assert idx[-1, :3].tolist() == [48, 49, 50] and (dist[-1, :3] == 0).all()
    # 100 identical rows: more than 64 survivors of the filtering scan, so the slow selection runs, and no proof, so the fallback does
    same = np.repeat(R.unit_rows(10, 1, dim), 100, axis=0)
    (dist, idx, _), _ = _both(same, np.arange(100) * 1.0, q[:3], np.array([1000.0, 49.5, 4.5]), 0.0, 5, "100 identical rows")
    assert idx.tolist() == [[0, 1, 2, 3, 4]] * 3 and (dist[:, 1:] == dist[:, :1]).all()


@pytest.mark.parametrize("dim", DIMS)
def test_proof_failure_falls_back_to_the_exact_search(dim):
    rng = np.random.default_rng([11, dim])
    db = (1000.0 + 1e-3 * rng.normal(size=(200, dim))).astype(np.float32)
    q = (1000.0 + 1e-3 * rng.normal(size=(40, dim))).astype(np.float32)
    # the case proves something only if float32 |q|^2 + |d|^2 - 2 q.d picks other neighbours than float64 does
    exact = ((q.astype(np.float64)[:, None] - db.astype(np.float64)[None]) ** 2).sum(-1).argmin(1)
    gemm = ((q * q).sum(1, dtype=np.float32)[:, None] + (db * db).sum(1, dtype=np.float32)[None] - np.float32(2) * (q @ db.T)).argmin(1)
    assert (exact != gemm).any()
    along = np.arange(200) * 1.0
    (_, idx, count), _ = _both(db, along, q, np.linspace(120.0, 400.0, 40), 100.0, 5, "cancelling GEMM")
    full = count == 200
    assert full.any() and idx[full, 0].tolist() == exact[full].tolist()


@pytest.mark.parametrize("dim", DIMS)
def test_non_finite_descriptors_and_keys(dim):
    db, along = R.unit_rows(12, 150, dim).copy(), np.arange(150) * 10.0
    db[3, 1], db[70, 0], db[71, dim - 1], db[140, 2] = np.nan, np.inf, -np.inf, np.nan
    q = R.unit_rows(13, 12, dim).copy()
    q[4, 0], q[5, dim - 1] = np.nan, np.inf
    q_along = np.array([55.0, 755.0, 1455.0, 2000.0, 2000.0, 2000.0, np.nan, np.inf, -np.inf, -1.0, 0.0, 705.0])
    (dist, idx, count), _ = _both(db, along, q, q_along, 0.0, 8, "non-finite")
    assert count.tolist() == [6, 76, 146, 150, 150, 150, -1, -1, -1, 0, 1, 71]     # a query before the whole database: p = 0, count 0
    assert not np.isin(idx, [3, 70, 71, 140]).any()                          # never selected
    assert (idx[[4, 5, 6, 7, 8, 9]] == -1).all() and np.isinf(dist[[4, 5, 6, 7, 8, 9]]).all()      # select nothing / no answer by rule
    assert idx[0].tolist().count(-1) == 8 - 5                                # five finite rows among the six admissible
    # the self-search of the hurt trajectory: the NaN rows as queries AND as rows
    (_, idx, count), _ = _both(db, along, db, along, 20.0, 5, "non-finite self-search")
    assert (idx[[3, 70, 71, 140]] == -1).all() and not np.isin(idx, [3, 70, 71, 140]).any() and (count >= 0).all()
    # no database at all
    got = _raw(np.zeros((0, dim), np.float32), np.zeros(0), q, q_along, 0.0, 3)
    assert (got[1] == -1).all() and np.isinf(got[0]).all() and got[2].tolist() == [0, 0, 0, 0, 0, 0, -1, -1, -1, 0, 0, 0]


@pytest.mark.parametrize("dim", DIMS)
def test_whole_call_failures(dim):
    db, along = R.unit_rows(14, 200, dim), np.arange(200) * 10.0
    q, q_along = R.unit_rows(15, 130, dim), np.arange(130) * 15.0 + 40.0
    last = along.copy()
    last[-1] = last[-2] - 1e-9                                               # one decreasing pair, at the last position
    middle = along.copy()
    middle[100] = np.nan
    for what, bad in (("decreasing at the end", last), ("NaN in the middle", middle), ("Inf at the front", np.r_[-np.inf, along[1:]])):
        (dist, idx, count), _ = _both(db, bad, q, q_along, 30.0, 5, what)
        assert (count == -1).all() and (idx == -1).all() and np.isinf(dist).all() and (dist > 0).all()
    (_, _, count), _ = _both(db, np.r_[along[:-1], along[-2]], q, q_along, 30.0, 5, "a plateau at the end is no failure")
    assert (count >= 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_passes(dim):
    db, along = R.unit_rows(16, 300, dim), np.arange(300) * 10.0
    q, q_along = R.unit_rows(17, 300, dim), np.random.default_rng(18).uniform(-50.0, 3200.0, size=300)
    one, _ = _both(db, along, q, q_along, 100.0, 5, "300 x 300, the library's pass")
    for pass_queries in (128, 256):
        _equal(_raw(db, along, q, q_along, 100.0, 5, pass_queries), one, "pass_queries %d" % pass_queries)
    self_one, _ = _both(db, along, db, along, 100.0, 5, "self-search, the library's pass")
    _equal(_raw(db, along, db, along, 100.0, 5, 128), self_one, "self-search in three passes")


def test_two_runs_and_one_captured_graph_replayed_on_other_data():
    RT = H.pkg("retrieval")
    dev, T, dim, k = torch.device("cuda"), 129, 256, 5
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc, along = up(R.unit_rows(19, T, dim)), up(np.arange(T) * 10.0)
    first = [t.clone() for t in RT.revisit_search(desc, along, 25.0, k)]
    again = RT.revisit_search(desc, along, 25.0, k)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    _equal(tuple(t.cpu().numpy() for t in first), R.revisit_reference(_knn, desc, np.arange(T) * 10.0, desc, np.arange(T) * 10.0, 25.0, k), "eager")
    # another drive in the same buffers: other descriptors, a plateau, steps of 1 to 40 m
    desc2 = R.unit_rows(20, T, dim)
    along2 = np.cumsum(np.r_[0.0, np.random.default_rng(21).choice([0.0, 1.0, 12.5, 40.0], size=T - 1)])
    want2 = R.revisit_reference(_knn, up(desc2), along2, up(desc2), along2, 25.0, k)
    ws = torch.empty(H.pkg("lib").lib().epcnet_revisit_workspace_bytes(T, T, 0), dtype=torch.uint8, device=dev)
    RT.revisit_search(desc, along, 25.0, k, workspace=ws)                     # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = RT.revisit_search(desc, along, 25.0, k, workspace=ws)

    def replay(d, a):
        desc.copy_(up(d))
        along.copy_(up(a))
        g.replay()
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in out)

    _equal(replay(desc2, along2), want2, "replay on another drive")
    assert len(np.unique(want2[2])) > 20 and (np.diff(want2[2]) == 0).any()
    broken = along2.copy()
    broken[77] = broken[76] - 1.0
    dist, idx, count = replay(desc2, broken)                                 # one replay is a whole-call failure ...
    assert (count == -1).all() and (idx == -1).all() and np.isinf(dist).all()
    _equal(replay(desc2, along2), want2, "... and the next is whole again")


def test_revisit_index_in_pieces_equals_the_batch_call():
    RT, L = H.pkg("retrieval"), H.pkg("lib")
    dev, T, dim = torch.device("cuda"), 300, 256
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc, along = R.unit_rows(22, T, dim), np.cumsum(np.random.default_rng(23).choice([0.0, 5.0, 10.0], size=T))
    want = R.revisit_reference(_knn, up(desc), along, up(desc), along, 50.0, 5)
    batch = RT.revisit_search(up(desc), up(along), 50.0, 5)
    _equal(tuple(t.cpu().numpy() for t in batch), want, "batch")
    index = RT.RevisitIndex(T, dim=dim, min_travel=50.0, k=5, device=dev)
    parts, at = [], 0
    for m in (1, 7, 130, 1, 161):
        parts.append(index.add(up(desc[at:at + m]), up(along[at:at + m])))
        at += m
        assert len(index) == at and index.descriptors.shape == (at, dim) and index.along.shape == (at,)
    _equal(tuple(torch.cat([p[j] for p in parts]).cpu().numpy() for j in range(3)), want, "pieces of 1, 7, 130, 1 and 161")
    assert torch.equal(index.descriptors, up(desc)) and torch.equal(index.along, up(along))
    with pytest.raises(L.EpcNetError):                                       # beyond the capacity: never a reallocation
        index.add(up(desc[:1]), up(along[-1:]))
    assert len(index) == T
    with pytest.raises(L.EpcNetError):                                       # a float32 along is refused, never converted
        index.add(up(desc[:1]), up(along[-1:].astype(np.float32)))
    # a failed add stores its rows regardless; truncate drops them and the next add equals the batch result again
    index.truncate(139)
    dist, idx, count = index.add(up(desc[139:150]), up(along[139:150] - 1000.0))
    assert len(index) == 150 and (count == -1).all() and (idx == -1).all() and bool(torch.isinf(dist).all())
    index.truncate(139)
    got = index.add(up(desc[139:]), up(along[139:]))
    _equal(tuple(t.cpu().numpy() for t in got), tuple(w[139:] for w in want), "after truncate")
    with pytest.raises(L.EpcNetError):
        index.truncate(T + 1)
    with pytest.raises(L.EpcNetError):
        RT.revisit_search(up(desc), up(along.astype(np.float32)), 50.0)
    with pytest.raises(L.EpcNetError):
        RT.revisit_search(up(desc), up(along), 50.0, queries=up(desc))        # queries without q_along


def test_end_to_end_on_a_small_out_and_back_drive():
    RT, L = H.pkg("retrieval"), H.pkg("lib")
    dev = torch.device("cuda")
    eng, _ = H.make_engine("epc-net-l", O.seeded_weights("epc-net-l", 0), dev, in_flight=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # 40 scans 1 m apart, 20 out and 20 back along x; submaps of 2 m every 1 m: 38 submaps in 44 slots, the last six NaN descriptors
    S, length, spacing, slots = 40, 2.0, 1.0, 44
    poses = SR.identity_poses(S).reshape(S, 3, 4)
    poses[:, 0, 3] = np.minimum(np.arange(S), S - 1 - np.arange(S)).astype(np.float64)
    points, offsets = SR.pack([SR.scan(100 + i, 300) for i in range(S)])
    desc, status, _, num_out = eng.forward_trajectory(up(points), up(offsets), up(poses.reshape(S, 12)), along=up(np.arange(S) * 1.0),
                                                      num_points=256, submaps=dict(length=length, spacing=spacing, max_submaps=slots,
                                                                                   out_rows=S * 300 * 3))
    K = int(num_out[0])
    status = status.cpu().numpy()
    assert 30 <= K < slots and (status[:K] == 0).all() and (status[K:] != 0).all() and bool(torch.isnan(desc[K:]).all())
    along = np.arange(slots) * spacing
    dist, idx, count = (t.cpu().numpy() for t in RT.revisit_search(desc, up(along), 3 * length, 5))
    want = R.revisit_reference(_knn, desc, along, desc, along, 3 * length, 5)
    _equal((dist, idx, count), want, "the drive's descriptors")
    assert count.tolist() == R.prefix_counts(along, along, 3 * length).tolist() and (count[S // 2:K] > 0).all()     # the return leg
    assert (idx[K:] == -1).all() and (idx < K).all()                         # a NaN slot selects nothing and is never selected
    assert (idx[7:K, 0] >= 0).all()


def test_no_query_with_the_callers_workspace_and_with_none():
    """Q = 0 queries against T = 8 rows of dim 8: the empty queries and outputs have no address, the workspace's stands in for them --
    the caller's, which nothing writes, or the entry's own."""
    RT = H.pkg("retrieval")
    dev = torch.device("cuda")
    desc = torch.from_numpy(R.unit_rows(5, 8, 8)).to(dev)
    along = torch.arange(8, dtype=torch.float64, device=dev)
    for ws in (torch.full((64,), 0xFF, dtype=torch.uint8, device=dev), None):
        dist, idx, count = RT.revisit_search(desc, along, 1.0, 3, queries=desc[:0], q_along=along[:0], workspace=ws)
        torch.cuda.synchronize()
        assert (tuple(dist.shape), tuple(idx.shape), tuple(count.shape)) == ((0, 3), (0, 3), (0,))
        assert (dist.dtype, idx.dtype, count.dtype) == (torch.float32, torch.int32, torch.int32)
        assert ws is None or bool((ws == 0xFF).all())
