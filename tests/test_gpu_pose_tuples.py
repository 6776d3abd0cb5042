"""Relations and training tuples from poses on the device (csrc/pose_tuples.hip; ops.PoseTuples, ops.pose_radius_lists,
retrieval.truth_from_poses, utils.loading_pointclouds.query_dict_from_poses, TrainStep.step_ids with device ids,
Trainer(poses=...)).  Every comparison with tests/tuples_ref.py is bit for bit -- ids, counts and status words; no tolerance anywhere.
The fixture's poses lie on a 1/8 m lattice (exact float64 distances), include pairs at exactly 10, 25 and 50 m, and collapse onto a
0.5 m lattice in float32, so a float32 shortcut or a wrong edge shows here."""
import logging

import numpy as np
import pytest
import torch

import helpers as H
import tuples_ref as R

pytestmark = pytest.mark.gpu
R_POS, R_NEG = 10.0, 50.0
SIZES = [257, 1000, 5003]       # no multiple of a wave or a workgroup; 5003: more than one pass per thread of the 1024


@pytest.fixture
def dev():
    return torch.device("cuda:0")


_POSES = {}


def _poses(T):
    if T not in _POSES:
        _POSES[T] = R.fixture_poses(T)           # (shared: no test writes to it)
    return _POSES[T]


def _keys(T):
    """The hand-placed records (edges, duplicates, the cluster) and records along the loop, the last one included."""
    return [0, 1, 4, 5, 6, 8, 11, 12, 31, 32, T // 2, T - 1]


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)


def _dist2(poses, a, b):
    dx, dy = poses[a, 0] - poses[b, 0], poses[a, 1] - poses[b, 1]
    return dx * dx + dy * dy


def _assert_tuple_relations(poses, row, P, Nn, hard=()):
    """The reference's relations for one drawn tuple {key, positives, negatives, other}, by brute force (not through tuples_ref)."""
    T = len(poses)
    key, pos, neg, other = int(row[0]), [int(c) for c in row[1:1 + P] if c >= 0], [int(c) for c in row[1 + P:1 + P + Nn] if c >= 0], int(row[-1])
    assert all(c != key and _dist2(poses, c, key) <= 100.0 for c in pos), (key, pos)
    assert all(_dist2(poses, c, key) > 2500.0 for c in neg if c not in hard), (key, neg)
    assert len(set(pos)) == len(pos) and len(set(neg)) == len(neg)
    if other >= 0:
        near = lambda c, o: c != o and _dist2(poses, c, o) <= 100.0          # "c is a positive of o"
        assert 0 <= other < T and not near(other, key) and not any(near(other, n) for n in neg), (key, other)


@pytest.mark.parametrize("T", SIZES)
def test_pos_count_and_radius_lists(dev, T):
    ops = H.pkg("ops")
    poses = _poses(T)
    pt = ops.PoseTuples(poses, R_POS, R_NEG, device=dev)
    assert np.array_equal(pt.counts.cpu().numpy(), R.pos_count(poses, R_POS))
    q = poses[:64]
    for r in (10.0, 25.0, 50.0):
        padded, lens = ops.pose_radius_lists(q, poses, r, device=dev)
        want_pad, want_len, _ = R.radius_tables(q, poses, r)
        assert padded.dtype == torch.int32 and np.array_equal(lens.cpu().numpy(), want_len) and np.array_equal(padded.cpu().numpy(), want_pad)
    # the inclusive / exclusive edges and the float32 collapse, said directly
    lists = lambda r: [row[row >= 0].tolist() for row in ops.pose_radius_lists(poses[:8], poses[:8], r, device=dev)[0].cpu().numpy()]
    assert lists(10.0)[0] == [0, 1] and lists(25.0)[2] == [2, 3] and lists(50.0)[4] == [4, 5] and lists(10.0)[6] == [6]
    p32 = poses.astype(np.float32).astype(np.float64)
    assert not np.array_equal(R.pos_count(p32, R_POS), pt.counts.cpu().numpy())


def _few_negatives_poses():
    """50 consecutive loop records 2.5 m apart (a 125 m stretch): every key has fewer than 64 negatives."""
    return np.ascontiguousarray(_poses(5003)[1000:1050])


@pytest.mark.parametrize("case", ["257-C64", "1000-C64", "few-negatives-C64", "5003-C4000"])
def test_candidates_equal_the_restatement_and_feed_mine_topk(dev, case):
    ops, RT = H.pkg("ops"), H.pkg("retrieval")
    if case == "few-negatives-C64":
        poses, C, keys = _few_negatives_poses(), 64, [0, 25, 49]
    else:
        T, C = int(case.split("-")[0]), int(case.split("-C")[1])
        poses, keys = _poses(T), (_keys(T) if C == 64 else [0, 12, T - 1])
    T = len(poses)
    pt = ops.PoseTuples(poses, R_POS, R_NEG, seed=5, device=dev)
    for B, step in ((1, 0), (3, 2 ** 40 + 9)):
        for a in range(0, len(keys) - B + 1, B):
            ks = keys[a:a + B]
            cand, count = pt.candidates(_i32(ks, dev), step, C)
            want, _ = R.candidates(poses, ks, R_NEG, 5, step, C)
            got, n = cand.cpu().numpy(), count.cpu().numpy()
            for b in range(B):
                assert n[b] == len(want[b]) and np.array_equal(got[b, :n[b]], want[b]), (case, ks[b])
                negatives = int(R.negatives_mask(poses, ks[b], R_NEG).sum())
                assert n[b] == min(C, negatives) and (case != "few-negatives-C64" or n[b] < C) and (case == "few-negatives-C64" or negatives > C)
    pt.check()
    # the buffers go to mine_topk as they are: its ids are the nearest rows among exactly these candidates
    rng = np.random.RandomState(1)
    table = rng.randn(T, 16).astype(np.float32)
    ks = keys[:3]
    cand, count = pt.candidates(_i32(ks, dev), 7, C)
    queries = table[ks] + 0.1 * rng.randn(3, 16).astype(np.float32)
    k = 10
    _, pos, ids = RT.mine_topk(torch.from_numpy(table).to(dev), torch.from_numpy(queries).to(dev), cand, count, k)
    want, _ = R.candidates(poses, ks, R_NEG, 5, 7, C)
    for b in range(3):
        d = ((table[want[b]].astype(np.float64) - queries[b].astype(np.float64)) ** 2).sum(1)
        order = np.argsort(d, kind="stable")[:k]
        assert ids[b].cpu().numpy()[:len(order)].tolist() == want[b][order].tolist()


@pytest.mark.parametrize("T", SIZES)
def test_sample_equals_the_restatement(dev, T):
    """P = 2, Nn = 14 without hard negatives, B = 1 and B = 3, two steps (one beyond 2^32); keys 0 and 1 have P - 1 positives, keys 4, 5
    and 6 none (status bit, -1 slots), keys 8..11 more than P."""
    ops = H.pkg("ops")
    poses = _poses(T)
    pt = ops.PoseTuples(poses, R_POS, R_NEG, seed=(7 << 32) + 3, device=dev)
    P, Nn = 2, 14
    keys = _keys(T)
    for B, step in ((1, 0), (3, 2 ** 33 + 1)):
        for a in range(0, len(keys) - B + 1, B):
            ks = keys[a:a + B]
            ids, _ = pt.sample(_i32(ks, dev), step, P, Nn)
            want, want_status = R.sample(poses, ks, R_POS, R_NEG, (7 << 32) + 3, step, P, Nn)
            got = ids.cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, want), (T, ks, got, want)
            for row in got:
                _assert_tuple_relations(poses, row, P, Nn)
    with pytest.raises(H.pkg("lib").EpcNetError) as e:       # per slot the LAST key that set a bit: 6 of the B = 1 calls; 5, 6, 4 of B = 3
        pt.check()
    assert "key 6 (slot 0 of 1): fewer positives" in str(e.value) and "key 4 (slot 2 of 3): fewer positives" in str(e.value)
    pt.check()                                               # cleared


def test_sample_statuses_and_edges(dev):
    ops, L = H.pkg("ops"), H.pkg("lib")
    T = 1000
    poses = _poses(T)
    pt = ops.PoseTuples(poses, R_POS, R_NEG, seed=1, device=dev)

    def both(keys, step, P, Nn, hard=None, p=poses, t=pt):
        ids, status = t.sample(_i32(keys, dev), step, P, Nn, hard=None if hard is None else _i32(hard, dev))
        want, want_status = R.sample(p, keys, R_POS, R_NEG, t.seed, step, P, Nn, hard=hard)
        got, st = ids.cpu().numpy(), status.cpu().numpy().copy()
        status.zero_()
        assert np.array_equal(got, want) and np.array_equal(st, want_status), (keys, got, want, st, want_status)
        return got, st

    # exactly P positives (key 0 has one, keys 8..11 three each) and P - 1
    got, st = both([0], 3, 1, 14)
    assert st.tolist() == [0] and got[0, 1] == 1
    got, st = both([8], 3, 3, 14)
    assert st.tolist() == [0] and sorted(got[0, 1:4].tolist()) == [9, 10, 11]
    got, st = both([0, 8, 500], 4, 2, 14)
    assert st.tolist() == [L.EPC_TUPLE_FEW_POSITIVES, 0, 0] and got[0, 1:3].tolist() == [1, -1]
    # hard ids with -1 entries, a repeat, an id outside the records; more hard ids than Nn
    hard = [[700, -1, 700, 650, T, -1, 600, -1], [-1] * 8, [5, 6, 7, 5, -1, 640, 641, 642]]
    got, st = both([40, 41, 300], 5, 2, 6, hard=hard)
    assert got[0, 3:6].tolist() == [700, 650, 600] and got[2, 3:9].tolist() == [5, 6, 7, 640, 641, 642]
    for row, h in zip(got, hard):
        _assert_tuple_relations(poses, row, 2, 6, hard=h)
    got, st = both([40], 5, 2, 3, hard=[[700, 650, 600, 610, 620]])
    assert got[0, 3:6].tolist() == [700, 650, 600]
    # a key outside [0, T): every slot -1; check() names it
    got, st = both([T, 40, -1], 6, 2, 14)
    assert (got[0] == -1).all() and (got[2] == -1).all() and st.tolist() == [L.EPC_TUPLE_BAD_KEY, 0, L.EPC_TUPLE_BAD_KEY]
    pt.sample(_i32([T], dev), 6, 2, 14)
    with pytest.raises(L.EpcNetError) as e:
        pt.check()
    assert "key %d " % T in str(e.value) and "outside" in str(e.value)
    # fewer than Nn negatives: the 125 m stretch
    few = _few_negatives_poses()
    pt_few = ops.PoseTuples(few, R_POS, R_NEG, seed=1, device=dev)
    negatives = int(R.negatives_mask(few, 25, R_NEG).sum())
    assert 0 < negatives < 14
    got, st = both([25, 0], 1, 2, 14, p=few, t=pt_few)
    assert st[0] == L.EPC_TUPLE_FEW_NEGATIVES and (got[0, 3:3 + negatives] >= 0).all() and (got[0, 3 + negatives:17] == -1).all()
    # The 20-record cluster alone (records 12..31, all within 10 m): every other record is a positive of the key.  The key itself stays
    # eligible by the reference's rule (nobody is his own positive) -- until a "negative" handed in as hard is one of its neighbours.
    cluster = np.ascontiguousarray(poses[12:32])
    pt_c = ops.PoseTuples(cluster, R_POS, R_NEG, seed=1, device=dev)
    assert pt_c.counts.cpu().tolist() == [19] * 20
    got, st = both([4], 2, 2, 3, p=cluster, t=pt_c)
    assert st.tolist() == [L.EPC_TUPLE_FEW_NEGATIVES] and got[0, 3:6].tolist() == [-1] * 3 and got[0, 6] == 4
    got, st = both([4], 2, 2, 3, hard=[[9, -1]], p=cluster, t=pt_c)
    assert st.tolist() == [L.EPC_TUPLE_FEW_NEGATIVES | L.EPC_TUPLE_NO_OTHER] and got[0, 3:7].tolist() == [9, -1, -1, -1]
    pt_c.sample(_i32([4], dev), 2, 2, 3, hard=_i32([[9, -1]], dev))
    with pytest.raises(L.EpcNetError) as e:
        pt_c.check()
    assert "key 4 " in str(e.value) and "no eligible other negative" in str(e.value) and "fewer negatives" in str(e.value)


def test_sample_with_hard_ids_from_mine_topk(dev):
    """candidates -> mine_topk (k = 10) -> sample, everything staying on the device; B = 3."""
    ops, RT = H.pkg("ops"), H.pkg("retrieval")
    T, P, Nn, step = 1000, 2, 14, 11
    poses = _poses(T)
    pt = ops.PoseTuples(poses, R_POS, R_NEG, seed=2, device=dev)
    keys = [40, 500, 999]
    kd = _i32(keys, dev)
    rng = np.random.RandomState(3)
    table = torch.from_numpy(rng.randn(T, 32).astype(np.float32)).to(dev)
    cand, count = pt.candidates(kd, step, 64)
    _, _, mined = RT.mine_topk(table, table[kd.long()].contiguous(), cand, count, 10)
    ids, status = pt.sample(kd, step, P, Nn, hard=mined)
    hard = mined.cpu().numpy()
    want, want_status = R.sample(poses, keys, R_POS, R_NEG, 2, step, P, Nn, hard=hard.tolist())
    got = ids.cpu().numpy()
    assert np.array_equal(got, want) and status.cpu().tolist() == [0, 0, 0]
    for b in range(3):
        assert (hard[b] >= 0).all() and got[b, 3:13].tolist() == hard[b].tolist()
        assert R.negatives_mask(poses, keys[b], R_NEG)[hard[b]].all()
        _assert_tuple_relations(poses, got[b], P, Nn)
    pt.check()


def _runs():
    p = _poses(300)
    # the 25.0 m pair (records 2, 3) sits across runs in both directions
    return [np.concatenate([p[2:4], p[32:70]]), np.concatenate([p[3:4], p[2:3], p[45:113]]), np.ascontiguousarray(p[32:161])]


def test_truth_from_poses_equals_packed_brute_force(dev):
    ops, RT, L = H.pkg("ops"), H.pkg("retrieval"), H.pkg("lib")
    runs = _runs()
    assert [len(r) for r in runs] == [40, 70, 129]

    def truth(m, n):
        return [[int(j) for j in range(len(runs[m])) if (runs[m][j, 0] - q[0]) ** 2 + (runs[m][j, 1] - q[1]) ** 2 <= 625.0] for q in runs[n]]
    want = RT.pack_truth(truth, [len(r) for r in runs], [len(r) for r in runs])
    got = RT.truth_from_poses(runs, runs, r=25.0, device=dev)
    assert got.n_dbs == want.n_dbs and got.n_qs == want.n_qs and got.device == dev
    for m in range(3):
        assert got.padded[m].dtype == torch.int32 and got.lens[m].dtype == torch.int32
        assert torch.equal(got.padded[m].cpu(), want.padded[m]) and torch.equal(got.lens[m].cpu(), want.lens[m])
    assert 0 in truth(1, 0)[0] and 0 in truth(0, 1)[0]       # records 2 and 3, exactly 25.0 m apart: true neighbours both ways
    rng = np.random.RandomState(0)
    vec = [rng.randn(len(r), 256).astype(np.float32) for r in runs]
    a = RT.evaluate_runs(vec, vec, truth, device=dev)
    b = RT.evaluate_runs(vec, vec, got, device=dev)
    assert a.keys() == b.keys() and np.array_equal(a["ave_recall"], b["ave_recall"])
    assert a["average_similarity"] == b["average_similarity"] and a["ave_one_percent_recall"] == b["ave_one_percent_recall"]
    # a width that is too small: the status word is set, the rows are truncated, lens keep the full lengths
    longest = int(max(t.max() for t in want.lens))
    assert longest > 3
    with pytest.raises(L.EpcNetError) as e:
        ops.pose_radius_lists(runs[0], runs[2], 25.0, width=3, device=dev)
    assert "truncated" in str(e.value)
    import ctypes
    q, d = torch.from_numpy(runs[0]).to(dev), torch.from_numpy(runs[2]).to(dev)
    lens = torch.zeros(40, dtype=torch.int32, device=dev)
    padded = torch.full((40, 4), 77, dtype=torch.int32, device=dev)     # (one column more than the width: it must stay untouched)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rad = ctypes.c_double(25.0)
    L.run.epcnet_pose_radius_fill(q, 40, d, 129, ctypes.byref(rad), 3, lens, padded, status)
    want_pad, want_len, want_status = R.radius_tables(runs[0], runs[2], 25.0, width=3)
    assert int(status.item()) == 1 == want_status and np.array_equal(lens.cpu().numpy(), want_len)
    flat = padded.cpu().numpy().reshape(-1)
    assert np.array_equal(flat[:120].reshape(40, 3), want_pad) and (flat[120:] == 77).all()


def test_query_dict_from_poses_is_the_brute_force_dict(dev):
    LP = H.pkg("utils.loading_pointclouds")
    poses = _poses(300)
    got = LP.query_dict_from_poses(poses, R_POS, R_NEG)
    assert got == R.brute_force_dict(poses, R_POS, R_NEG)


def test_refusals(dev):
    ops, L, TL = H.pkg("ops"), H.pkg("lib"), H.pkg("train_loop")
    poses = _poses(257)
    for bad in (poses.astype(np.float32), torch.from_numpy(poses).float().to(dev), poses[:, :1], poses.astype(np.int64)):
        with pytest.raises(L.EpcNetError):
            ops.PoseTuples(bad, device=dev)
    with pytest.raises(L.EpcNetError):
        ops.pose_radius_lists(poses.astype(np.float32), poses, 25.0, device=dev)
    pt = ops.PoseTuples(torch.from_numpy(poses).to(dev))
    keys = _i32([3], dev)
    for call in (lambda: pt.candidates(keys, 0, 4097), lambda: pt.candidates(keys, 0, 0), lambda: pt.sample(keys, 0, 40, 23),
                 lambda: pt.sample(keys, 0, 2, 14, hard=torch.zeros((1, 33), dtype=torch.int32, device=dev)),
                 lambda: pt.sample(torch.tensor([3], device=dev), 0, 2, 14), lambda: pt.sample(keys.cpu(), 0, 2, 14)):
        with pytest.raises(L.EpcNetError):
            call()
    pt.check()
    with pytest.raises(ValueError):
        TL.Trainer(None, None, np.zeros((257, 64, 3), np.float32), bank=True, device_mining=False, poses=poses)
    with pytest.raises(ValueError):
        TL.Trainer(None, None, np.zeros((257, 64, 3), np.float32), bank=False, device_mining=False, poses=poses)


# ---- the training step and the loop -------------------------------------------------------------------------------------------------
N_POINTS = 256


def _clouds(T, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (T, N_POINTS, 3)).astype(np.float32)


def _step(dev, nq=1, P=2, Nn=6):
    V, TR = H.pkg("variables"), H.pkg("training")
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=nq, POSITIVES_PER_QUERY=P, NEGATIVES_PER_QUERY=Nn, NUM_POINTS=N_POINTS,
                  BASE_LEARNING_RATE=1e-3, MAX_EPOCH=8)
    st = V.reset_default_store(device=dev, seed=0)
    ts = TR.TrainStep(params, st)
    ts._ensure_built(N_POINTS)
    st.randomize_statistics(0)
    return ts


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_step_ids_with_device_ids_is_the_same_step(dev, graph):
    """Four int32 device tensors -- slices of one sampled tensor, or separate tensors -- against the same ids as numpy arrays: the same
    loss bits over three steps (with graph=True: a capture and two replays that must pick up the refreshed ids)."""
    ops = H.pkg("ops")
    T, B, P, Nn = 40, 2, 2, 6
    data = torch.from_numpy(_clouds(T)).to(dev)
    rng = np.random.RandomState(4)
    sets = [rng.randint(0, T, (B, 1 + P + Nn + 1)).astype(np.int32) for _ in range(3)]
    split = lambda f: (f[:, :1], f[:, 1:1 + P], f[:, 1 + P:1 + P + Nn], f[:, 1 + P + Nn:])
    runs = []
    for form in ("numpy", "device-slices", "device-separate"):
        ts = _step(dev, nq=B, P=P, Nn=Nn)
        bank = ops.CloudBank(N_POINTS, T, dev)
        bank.add(data)
        losses = []
        for f in sets:
            if form == "numpy":
                parts = split(f)
            elif form == "device-slices":
                parts = split(torch.from_numpy(f).to(dev))
            else:
                parts = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in split(f))
            loss, _, _ = ts.step_ids(bank, *parts, epoch=1, graph=graph)
            losses.append(np.float32(float(loss)).view(np.uint32))
        bank.check()
        runs.append(losses)
    assert all(np.isfinite(np.array(r, dtype=np.uint32).view(np.float32)).all() for r in runs)
    assert runs[0] == runs[1] == runs[2] and len(set(int(v) for v in runs[0])) == 3


def _loop_poses():
    """60 records 2.5 m apart along the loop (150 m: every key has positives and at least 6 negatives), the last one moved 1 km away:
    no positives, so it leaves the epoch."""
    p = np.ascontiguousarray(_poses(5003)[2000:2060]).copy()
    p[59] += 1000.0
    return p


def test_trainer_from_poses(dev, tmp_path):
    """Trainer(poses=...) with a descriptor cache present (the mining runs): finite losses, every tuple stepped on obeys the relations
    by brute force, hard negatives come first; the same tuple_seed repeats the run bit for bit, another seed draws other tuples."""
    TL = H.pkg("train_loop")
    T, P, Nn = 60, 2, 6
    poses, data = _loop_poses(), _clouds(60, seed=1)

    def run(seed):
        ts = _step(dev, nq=1, P=P, Nn=Nn)
        log = logging.getLogger("pose-tuples-%d" % seed)
        log.setLevel(logging.INFO)
        lines = []
        handler = logging.Handler()
        handler.emit = lambda rec: lines.append(rec.getMessage())
        log.addHandler(handler)
        tr = TL.Trainer(ts, None, data, logger=log, bank=True, device_mining=True, poses=poses, tuple_seed=seed)
        stepped = []
        inner = ts.step_ids

        def spy(bank, q, pos, neg, oth, **kw):
            assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.int32 for x in (q, pos, neg, oth))
            stepped.append(torch.cat([q, pos, neg, oth], 1).cpu().numpy().copy())
            return inner(bank, q, pos, neg, oth, **kw)
        ts.step_ids = spy
        np.random.seed(0)
        tr.TRAINING_LATENT_VECTORS = tr.get_latent_vectors()
        losses = tr.train_one_epoch(6, max_iters=6)
        tr.tuples.check()
        log.removeHandler(handler)
        return losses, np.concatenate(stepped), lines

    a, b, c = run(0), run(0), run(12345)
    assert len(a[0]) == 6 and all(np.isfinite(a[0])) and all(np.isfinite(c[0]))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])                       # equal floats, equal tuples
    assert not np.array_equal(a[1], c[1]) and np.array_equal(a[1][:, 0], c[1][:, 0])     # the same keys (np.random), other draws
    assert any("1 of 60 keys have fewer than 2 positives" in m for m in a[2])
    for rows in (a[1], c[1]):
        assert rows.shape == (6, 1 + P + Nn + 1) and (rows >= 0).all() and 59 not in rows[:, 0]
        for row in rows:
            _assert_tuple_relations(poses, row, P, Nn)
