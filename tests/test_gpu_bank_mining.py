"""Hard-negative mining on the device (csrc/retrieval.hip: epc_mine_topk, retrieval.mine_topk, Trainer(bank=True,
device_mining=True)).  The search over rows named by id equals the search over the gathered rows bit for bit -- positions, ids and
distances as int32 bit patterns -- and a seeded training run mines the same negatives and steps alike.  No tolerance anywhere."""
import logging
import random

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
ROWS, DIM = 600, 256


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _table():
    """600 x 256 unit rows; 12 rows are exact copies of other rows (ties), 3 rows NaN, one +Inf."""
    rng = np.random.RandomState(0)
    t = rng.randn(ROWS, DIM).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    src, dst = np.arange(100, 112), np.arange(300, 312)
    t[dst] = t[src]
    t[[7, 205, 599]] = np.nan
    t[[50]] = np.inf
    return t, src, dst


def _pairwise_topk(db, q, k):
    """epc_pairwise_topk on (rows, D) x (1, D) with k = min(k, rows), padded to k with (-1, +inf)."""
    L = H.pkg("lib")
    kk = min(k, int(db.shape[0]))
    idx = torch.full((1, k), -1, dtype=torch.int32, device=db.device)
    dist = torch.full((1, k), float("inf"), dtype=torch.float32, device=db.device)
    i2 = torch.empty((1, kk), dtype=torch.int32, device=db.device)
    d2 = torch.empty((1, kk), dtype=torch.float32, device=db.device)
    L.check(L.lib().epc_pairwise_topk(db.data_ptr(), int(db.shape[0]), q.data_ptr(), 1, int(db.shape[1]), kk, i2.data_ptr(),
                                      d2.data_ptr(), L.current_stream()))
    idx[:, :kk], dist[:, :kk] = i2, d2
    return dist, idx


def _reference(table, queries, cand, counts, k):
    """Per query: gather the candidate rows with torch (an id outside the table: a NaN row, never selected) and search them."""
    R = int(table.shape[0])
    dist, pos, ids = [], [], []
    for q in range(int(queries.shape[0])):
        c = cand[q, :counts[q]].long()
        ok = (c >= 0) & (c < R)
        rows = table[c.clamp(0, R - 1)].clone()
        rows[~ok] = float("nan")
        d, p = _pairwise_topk(rows.contiguous(), queries[q:q + 1].contiguous(), k)
        i = torch.where(p >= 0, cand[q][p.clamp(min=0).long()], torch.full_like(p, -1))
        dist.append(d), pos.append(p), ids.append(i)
    return torch.cat(dist), torch.cat(pos), torch.cat(ids)


def _candidates(rng, count, src, dst):
    if count >= ROWS:                                       # more candidates than rows: repeats of ids
        c = rng.randint(0, ROWS, count)
    else:
        c = rng.permutation(ROWS)[:count]
    if count >= 64:                                         # both copies of the tied rows, the copy FIRST for half of them
        c[:12] = np.where(np.arange(12) % 2 == 0, src, dst)
        c[20:32] = np.where(np.arange(12) % 2 == 0, dst, src)
        c[40], c[41] = ROWS, -1                             # ids outside the table
        c[42], c[43] = 7, 50                                # a NaN row and the +Inf row
    return c.astype(np.int32)


@pytest.mark.parametrize("counts", [[4000], [257], [64], [10], [7], [4000, 257, 7], [64, 10, 4000]], ids=lambda c: "x".join(map(str, c)))
def test_mine_topk_equals_search_over_gathered_rows(dev, counts):
    R = H.pkg("retrieval")
    t_np, src, dst = _table()
    table = torch.from_numpy(t_np).to(dev)
    rng = np.random.RandomState(len(counts) * 100 + counts[0])
    Q, k = len(counts), 10
    C = max(counts) + 5
    qs = t_np[src[1:1 + Q]].copy()                          # the query IS a tied row: distance 0 to both copies
    if Q == 3:
        qs[1] = np.nan                                      # one query is a NaN row
        qs[2] = (qs[2] + 0.05 * rng.randn(DIM)).astype(np.float32)
    cand = np.full((Q, C), int(src[0]), dtype=np.int32)     # beyond the count: a row at distance 0 that must never be read
    for q, n in enumerate(counts):
        cand[q, :n] = _candidates(rng, n, src, dst)
    queries = torch.from_numpy(qs).to(dev)
    cand_t = torch.from_numpy(cand).to(dev)
    cnt_t = torch.tensor(counts, dtype=torch.int32, device=dev)
    dist, pos, ids = R.mine_topk(table, queries, cand_t, cnt_t, k)
    wd, wp, wi = _reference(table, queries, cand_t, counts, k)
    assert torch.equal(pos, wp) and torch.equal(ids, wi)
    assert torch.equal(dist.view(torch.int32), wd.view(torch.int32))
    pos_h, ids_h, dist_h = pos.cpu().numpy(), ids.cpu().numpy(), dist.cpu().numpy()
    for q, n in enumerate(counts):
        assert (pos_h[q] < n).all()
        live = pos_h[q] >= 0
        assert not np.isin(ids_h[q][live], [ROWS, -1, 7, 50]).any()
        assert np.isinf(dist_h[q][~live]).all() and (ids_h[q][~live] == -1).all()
        if n < k:
            assert (~live[n:]).all()                        # count < k: (-1, +inf) tails
        if np.isnan(qs[q]).any():
            assert (~live).all()
        elif n >= 64 and q == 0:
            # the query equals the tied rows of pair 1, whose COPY (the higher id) stands first in the list: both at distance 0,
            # the lower position first -- not the lower id
            assert dist_h[q][0] == 0.0 and dist_h[q][1] == 0.0
            assert (int(pos_h[q][0]), int(pos_h[q][1])) == (1, 21) and (int(ids_h[q][0]), int(ids_h[q][1])) == (int(dst[1]), int(src[1]))


def test_mine_topk_small_dim_largest_k(dev):
    """dim = 8, k = 56, count = 56: every candidate comes back, sorted."""
    R = H.pkg("retrieval")
    rng = np.random.RandomState(5)
    table = torch.from_numpy(rng.randn(90, 8).astype(np.float32)).to(dev)
    queries = torch.from_numpy(rng.randn(2, 8).astype(np.float32)).to(dev)
    cand = torch.from_numpy(np.stack([rng.permutation(90)[:56], rng.permutation(90)[:56]]).astype(np.int32)).to(dev)
    counts = [56, 56]
    dist, pos, ids = R.mine_topk(table, queries, cand, torch.tensor(counts, dtype=torch.int32, device=dev), 56)
    wd, wp, wi = _reference(table, queries, cand, counts, 56)
    assert torch.equal(pos, wp) and torch.equal(ids, wi) and torch.equal(dist.view(torch.int32), wd.view(torch.int32))
    assert sorted(pos[0].tolist()) == list(range(56))


def test_against_numpy_brute_force(dev):
    """A tie-free random table against a float64 brute force, indices only -- for the mining form and for epc_pairwise_topk, whose
    row distance is now the shared device function."""
    R = H.pkg("retrieval")
    rng = np.random.RandomState(9)
    t = rng.randn(500, DIM).astype(np.float32)
    qs = rng.randn(4, DIM).astype(np.float32)
    cand = np.stack([rng.permutation(500)[:300] for _ in range(4)]).astype(np.int32)
    table, queries = torch.from_numpy(t).to(dev), torch.from_numpy(qs).to(dev)
    _, pos, ids = R.mine_topk(table, queries, torch.from_numpy(cand).to(dev), torch.full((4,), 300, dtype=torch.int32, device=dev), 10)
    for q in range(4):
        d = ((t[cand[q]].astype(np.float64) - qs[q].astype(np.float64)) ** 2).sum(1)
        order = np.argsort(d, kind="stable")[:10]
        assert pos[q].tolist() == order.tolist() and ids[q].tolist() == cand[q][order].tolist()
        full = ((t.astype(np.float64) - qs[q].astype(np.float64)) ** 2).sum(1)
        _, idx = _pairwise_topk(table, queries[q:q + 1].contiguous(), 25)
        assert idx[0].tolist() == np.argsort(full, kind="stable")[:25].tolist()


def test_refusals(dev):
    """Outside the preconditions: EPC_EINVAL and nothing launched (the outputs keep their contents)."""
    L = H.pkg("lib")
    lib = L.lib()
    table = torch.zeros((ROWS, DIM), dtype=torch.float32, device=dev)
    queries = torch.zeros((1, DIM), dtype=torch.float32, device=dev)
    cand = torch.zeros((1, 64), dtype=torch.int32, device=dev)
    count = torch.full((1,), 64, dtype=torch.int32, device=dev)
    pos = torch.full((1, 64), 77, dtype=torch.int32, device=dev)
    ids = torch.full((1, 64), 77, dtype=torch.int32, device=dev)
    dist = torch.full((1, 64), 77.0, dtype=torch.float32, device=dev)
    need = int(lib.epc_mine_topk_workspace_bytes(1, 64))
    assert need >= 64 * 4 and int(lib.epc_mine_topk_workspace_bytes(3, 4000)) >= 3 * 4000 * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(dim=DIM, max_cand=64, k=10, ws_bytes=need):
        return lib.epc_mine_topk(table.data_ptr(), ROWS, dim, queries.data_ptr(), 1, cand.data_ptr(), count.data_ptr(), max_cand, k,
                                 pos.data_ptr(), ids.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, L.current_stream())
    for kwargs in (dict(k=0), dict(k=57), dict(dim=6), dict(max_cand=16385, ws_bytes=1 << 30), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**kwargs) == L.EPC_EINVAL, kwargs
    torch.cuda.synchronize()
    assert bool((pos == 77).all()) and bool((ids == 77).all()) and bool((dist == 77.0).all())
    assert call() == L.EPC_OK
    torch.cuda.synchronize()
    assert pos[0, :10].tolist() == list(range(10))          # all rows equal the query: ties in position order


def _dataset(T, n, seed=0):
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1, 1, (T, n, 3)).astype(np.float32)
    queries = {}
    for i in range(T):
        queries[i] = {"query": "%d.bin" % i, "positives": [j for j in range(T) if j != i and abs(j - i) <= 2],
                      "negatives": [j for j in range(T) if abs(j - i) > 4]}
    return queries, data


class _Keep(logging.Handler):
    """Keeps the log lines; at every refresh of the descriptor cache (the handler runs before the next step changes the weights) it
    records whether the cache equals ``get_latent_vectors()`` and where it lives."""

    def __init__(self):
        super().__init__()
        self.lines, self.tr, self.refreshes = [], None, []

    def emit(self, record):
        msg = record.getMessage()
        self.lines.append(msg)
        if "Updated cached feature vectors" in msg and self.tr is not None:
            cache = self.tr.TRAINING_LATENT_VECTORS
            on_device = torch.is_tensor(cache) and cache.is_cuda
            host = cache.cpu().numpy() if torch.is_tensor(cache) else np.asarray(cache)
            want = self.tr.get_latent_vectors()
            self.refreshes.append((on_device, host.dtype == np.float32 and np.array_equal(host.view(np.uint32), want.view(np.uint32))))


@pytest.mark.parametrize("nq", [1, 2])
def test_trainer_with_device_mining_is_the_same_run(dev, tmp_path, nq):
    """Trainer(bank=True, device_mining=True) against Trainer(bank=True) with the same seeds (the run of
    tests/test_gpu_cloud_bank.py::test_trainer_on_the_bank_is_the_same_run): the same mined negatives per key, the same losses (equal
    floats), skips, log lines and checkpoint tensors across a refresh of the descriptor cache, a save, a resume and two more steps."""
    V, TR, TL = H.pkg("variables"), H.pkg("training"), H.pkg("train_loop")
    N, T = 128, 40
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=nq, POSITIVES_PER_QUERY=2, NEGATIVES_PER_QUERY=6,
                  NUM_POINTS=N, BASE_LEARNING_RATE=1e-3, MAX_EPOCH=8)
    runs = []
    for on_device in (False, True):
        queries, data = _dataset(T, N)
        queries[5]["positives"] = [4]                          # fewer than P positives: "FAULTY TUPLE"
        st = V.reset_default_store(device=dev, seed=0)
        ts = TR.TrainStep(params, st)
        ts._ensure_built(N)
        st.randomize_statistics(0)
        log = logging.getLogger("mine-%d-%d" % (nq, on_device))
        log.setLevel(logging.INFO)
        keep = _Keep()
        log.addHandler(keep)
        save = str(tmp_path / ("mine%d" % on_device))
        tr = TL.Trainer(ts, queries, data, queries, data, save_path=save, logger=log, bank=True, device_mining=on_device)
        assert tr.bank is not None and tr.device_mining == on_device
        keep.tr = tr
        mined = []

        def spy(trainer):
            inner = trainer._hard_negatives
            trainer._hard_negatives = lambda key: (lambda h: (mined.append((int(key), list(h))), h)[1])(inner(key))
        spy(tr)
        np.random.seed(0)
        random.seed(0)
        tr.TRAINING_LATENT_VECTORS = tr.get_latent_vectors()    # numpy from the caller: the mining branch from the first iteration on
        losses = tr.train_one_epoch(6, max_iters=31 if nq == 1 else 16)      # crosses i == 29 (nq 1): the descriptor cache refresh
        tr.graph = True
        losses += tr.train_one_epoch(6, max_iters=4)
        tr.graph = False
        ev = tr.evaluate_loss(6)
        prefix = tr.save(6, 101)
        ckpt = tr.checkpoint_tensors()
        st2 = V.reset_default_store(device=dev, seed=123)
        ts2 = TR.TrainStep(params, st2)
        tr2 = TL.Trainer(ts2, queries, data, save_path=save, logger=log, bank=True, device_mining=on_device)
        spy(tr2)
        tr2.restore(prefix)
        tr2.TRAINING_LATENT_VECTORS = tr2.get_latent_vectors()
        losses += tr2.train_one_epoch(7, max_iters=2)
        ckpt2 = tr2.checkpoint_tensors()
        skips = [m.split("] ")[-1] for m in keep.lines if m.endswith("!!!")]
        runs.append((losses, ev, ckpt, ckpt2, skips, keep.refreshes, [m for m in keep.lines if "Loss" in m or m.endswith("!!!")], mined))
        log.removeHandler(keep)
    a, b = runs
    assert len(a[0]) >= 20 and all(np.isfinite(a[0]))
    assert a[0] == b[0] and a[1] == b[1]                       # the loss sequence and the evaluation loss: equal floats
    assert a[4] == b[4] and a[6] == b[6] and any("FAULTY TUPLE" in m for m in a[4])
    assert len(a[7]) >= 20 and all(len(h) == 10 for _, h in a[7]) and a[7] == b[7]   # the negatives each run mined, per key
    if nq == 1:
        # the slice crossed a refresh: the device run's cache is a device tensor holding exactly get_latent_vectors()
        assert len(a[5]) >= 1 and len(a[5]) == len(b[5])
        assert all(ok and not on_dev for on_dev, ok in a[5]) and all(ok and on_dev for on_dev, ok in b[5])
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k


def test_device_mining_needs_the_bank(dev):
    V, TR, TL = H.pkg("variables"), H.pkg("training"), H.pkg("train_loop")
    queries, data = _dataset(8, 128)
    st = V.reset_default_store(device=dev, seed=0)
    ts = TR.TrainStep(dict(H.PARAMS, ARCH="epc-net-l", NUM_POINTS=128), st)
    with pytest.raises(ValueError):
        TL.Trainer(ts, queries, data, bank=False, device_mining=True)
