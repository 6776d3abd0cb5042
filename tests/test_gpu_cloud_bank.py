"""The cloud bank (ops.CloudBank, csrc/graph_bank.hip): a training set resident in device memory as one record per cloud -- the sorted
cloud and its finished kNN graph with 16-bit indices -- and the step that assembles its batch from record ids (TrainStep.step_ids,
Trainer(bank=True)).  The bank changes where the graph comes from, never its content: EVERY comparison here is exact (torch.equal /
equal floats); the feature has no tolerance anywhere."""
import logging
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O

pytestmark = pytest.mark.gpu
CAP = 32


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _hub_cloud(n, seed, m=68):
    """A point with MORE than 64 points listing it (a transposed list longer than a wave: transpose_sort_kernel's one-lane form):
    m = 68 points evenly on the unit sphere around a centre point, everything else far away.  A sphere point has 0.25 m = 17 sphere
    points nearer than the centre (chord < 1 <=> angle < 60 degrees), so the centre is its 19th neighbour of 20: the centre is listed
    by the 68 and by itself.  (The in-degree of the other kinds stays below 40: measured with the oracle's lists.)"""
    rng = np.random.RandomState(seed)
    k = np.arange(m) + 0.5
    phi, th = np.arccos(1 - 2 * k / m), np.pi * (1 + 5 ** 0.5) * k
    shell = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1) * (1 + 1e-3 * rng.uniform(-1, 1, (m, 1)))
    rest = rng.uniform(-1, 1, (n - m - 1, 3)) + np.array([40.0, 0, 0])
    pc = np.concatenate([np.zeros((1, 3)), shell, rest], 0)
    return np.ascontiguousarray(pc[rng.permutation(n)][None], dtype=np.float32)


def _bank_clouds(n):
    """~40 clouds: ordinary ones and the hard kinds of tests/test_gpu_parity.py / test_gpu_knn_forms.py / test_gpu_train_ops.py."""
    parts = [O.synthetic_clouds(12, n, 1, "uniform"), O.synthetic_clouds(10, n, 2, "lidar"), O.synthetic_clouds(4, n, 3, "lattice"),
             O.synthetic_clouds(5, n, 4, "dup"), O.synthetic_clouds(2, n, 5, "zeros"), O.synthetic_clouds(3, n, 6, "zeropad25"),
             O.synthetic_clouds(2, n, 7, "repeat30"), _hub_cloud(n, 8), _hub_cloud(n, 9)]
    return np.concatenate(parts, 0)


def _fresh(xyz):
    """What the step builds today for the clouds ``xyz`` (T, n, 3)."""
    ops = H.pkg("ops")
    s = ops.morton_sort(xyz)
    g = ops.KnnGraph(s)
    rdeg, roff, rlist = g.transposed()
    oc, ol = g.overflow()
    return dict(xyz=s, kth=g.kth, cnt=g.cnt, idx=g.idx, rdeg=rdeg, roff=roff, rlist=rlist, ovf_cnt=oc, ovf_list=ol)


def _assert_same_graph(got_xyz, g, want, n):
    T = int(got_xyz.shape[0])
    assert g.num_clouds == T and g.n == n
    rdeg, roff, rlist = g.transposed()
    oc, ol = g.overflow()
    assert torch.equal(got_xyz, want["xyz"]) and g.xyz is got_xyz
    # (kth: the bits -- a zero-padded cloud's threshold is -0.0 / 0.0 and NaN never occurs; compare as integers to be strict)
    assert torch.equal(g.kth.view(torch.int32), want["kth"].view(torch.int32))
    assert torch.equal(g.cnt, want["cnt"])
    assert torch.equal(rdeg, want["rdeg"]) and torch.equal(roff, want["roff"]) and torch.equal(oc, want["ovf_cnt"])
    slot = torch.arange(CAP, device=got_xyz.device)[None, None, :]
    live = slot < want["cnt"].clamp(max=CAP)[:, :, None]               # the first min(cnt, cap) slots of every row
    assert g.idx.dtype == torch.int32 and torch.equal(g.idx[live], want["idx"][live])
    pos = torch.arange(T * n * CAP, device=got_xyz.device, dtype=torch.int64)
    # entries inside [roff, roff + rdeg): the lists of a cloud are packed from the start of its segment, so that is [seg, seg + used)
    used = (want["roff"].view(T, n)[:, -1] + want["rdeg"].view(T, n)[:, -1]).to(torch.int64)
    seg = torch.arange(T, device=got_xyz.device, dtype=torch.int64) * (n * CAP)
    inside = ((pos.view(T, -1) >= seg[:, None]) & (pos.view(T, -1) < used[:, None])).view(-1)
    assert int(inside.sum()) == int(want["rdeg"].sum())
    assert rlist.dtype == torch.int32 and torch.equal(rlist[inside], want["rlist"][inside])
    first = torch.arange(n, device=got_xyz.device)[None, :] < want["ovf_cnt"][:, None]
    assert torch.equal(ol[first], want["ovf_list"][first])


@pytest.mark.parametrize("n", [4096, 256])
def test_assemble_equals_fresh_build(dev, n):
    """assemble(ids) == morton_sort + KnnGraph + transposed() + overflow() on xyz[ids], exactly, for id lists with repeats and in
    scrambled order, into fresh buffers and into reused ones (stale contents of another batch underneath)."""
    ops = H.pkg("ops")
    data = torch.from_numpy(_bank_clouds(n)).to(dev)
    M = int(data.shape[0])
    bank = ops.CloudBank(n, M + 3, dev)
    assert bank.bytes_per_cloud == 16 + n * (28 + 4 * CAP + 2) and len(bank) == 0
    ids0 = bank.add(data[:17])
    ids1 = bank.add(data[17:])                      # (a second call appends)
    assert ids0 + ids1 == list(range(M)) and len(bank) == M
    # the bank really holds the hard cases: overflow rows (cnt > cap) and a transposed list longer than 64
    everything = _fresh(data)
    assert int((everything["cnt"] > CAP).sum()) > 0 and int(everything["ovf_cnt"].max()) > 0
    assert int(everything["rdeg"].max()) > 64
    assert 0 < int((everything["ovf_cnt"] > 0).sum()) < M
    rng = np.random.RandomState(0)
    lists = [list(range(M)), [M - 1, 0, M - 1, 5, 5, 5, 17], rng.permutation(M)[:18].tolist(), rng.randint(0, M, 22).tolist(),
             [int(i) for i in np.where(everything["ovf_cnt"].cpu().numpy() > 0)[0]] * 2, [3]]
    out18 = bank.buffers(18)
    for ids in lists:
        t = torch.tensor(ids, dtype=torch.int32, device=dev)
        want = _fresh(data[t.long()])
        xyz, g = bank.assemble(t)
        _assert_same_graph(xyz, g, want, n)
        if len(ids) == 18:
            for _ in range(2):                       # preallocated buffers: the same addresses every call
                ptr = out18["rlist"].data_ptr()
                xyz, g = bank.assemble(t.flip(0).contiguous(), out=out18)
                assert xyz is out18["xyz"] and g.transposed()[2].data_ptr() == ptr
                _assert_same_graph(xyz, g, _fresh(data[t.flip(0).long()]), n)
            xyz, g = bank.assemble(t, out=out18)     # ... over the stale contents of the flipped batch
            _assert_same_graph(xyz, g, want, n)
    bank.check()                                     # every id was valid: nothing to report
    # the records are a deterministic function of the clouds: a second bank built in another chunking holds the same bytes
    bank2 = ops.CloudBank(n, M + 3, dev)
    bank2.add(data)
    assert torch.equal(bank2.records[:M * bank.bytes_per_cloud], bank.records[:M * bank.bytes_per_cloud])


def _tuples(M, B, P, Nn, steps=3):
    """``steps`` id tuples (q (B,1), pos (B,P), neg (B,Nn), other (B,1)); the last differs from the one before it in ONE cloud only --
    a replay that did not pick up the refreshed ids would repeat the previous step.  Repeats inside a tuple occur."""
    rng = np.random.RandomState(11)
    T = 1 + P + Nn + 1
    out = []
    for s in range(steps):
        if s == steps - 1:
            flat = out[-1].copy()
            flat[B - 1, T - 2] = (flat[B - 1, T - 2] + 1 + rng.randint(0, M - 1)) % M
        else:
            flat = rng.randint(0, M, (B, T))
            flat[0, 2] = flat[0, 1]                  # the same cloud twice in a tuple
        out.append(flat)
    return [(f[:, :1], f[:, 1:1 + P], f[:, 1 + P:1 + P + Nn], f[:, T - 1:]) for f in out]


def _run_steps(dev, arch, prec, B, graph, data, tuples, use_ids, bad_first=False):
    """Three steps from the seeded initial state; returns (losses, every variable + Adam moment as numpy)."""
    TR, ops = H.pkg("training"), H.pkg("ops")
    params = dict(H.PARAMS, ARCH=arch, BATCH_NUM_QUERIES=B, TRAIN_PRECISION=prec, DECAY_STEP=2, BASE_LEARNING_RATE=1e-3)
    st = H.make_store(arch, O.seeded_weights(arch, 4), dev)
    ts = TR.TrainStep(params, st, outer=H.OUTER)
    n = int(data.shape[1])
    bank = None
    if use_ids:
        bank = ops.CloudBank(n, int(data.shape[0]), dev)
        bank.add(data)
    losses = []
    for i, tup in enumerate(tuples):
        if use_ids:
            loss, _, _ = ts.step_ids(bank, *tup, epoch=5 * i, graph=graph)
        else:
            q, pos, neg, oth = (data[torch.from_numpy(np.ascontiguousarray(x)).to(dev).long()] for x in tup)
            loss, _, _ = ts.step(q, pos, neg, oth, epoch=5 * i, graph=graph)
        losses.append(float(loss))
    torch.cuda.synchronize()
    ops.chain_persist_check()                        # (raises when a persistent chain launch was abandoned)
    if bank is not None:
        bank.check()
    state = {k: v.detach().cpu().numpy().copy() for k, v in st.vars.items()}
    state.update({k + "/Adam": v.detach().cpu().numpy().copy() for k, v in ts.m.items()})
    state.update({k + "/Adam_1": v.detach().cpu().numpy().copy() for k, v in ts.v.items()})
    assert ts.global_step == len(tuples)
    return losses, state


def _assert_same_run(a, b, what):
    (la, sa), (lb, sb) = a, b
    assert all(np.isfinite(la)), (what, la)
    assert la == lb, (what, la, lb)                                  # equal floats: the same bits
    assert len(set(la)) == len(la), (what, la)                       # (every step saw another tuple: step 3 is not step 2 again)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint32) if sa[k].dtype == np.float32 else sa[k],
                              sb[k].view(np.uint32) if sb[k].dtype == np.float32 else sb[k]), (what, k)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("prec", ["bf16", "bf16x6"])
@pytest.mark.parametrize("arch", ["epc-net", "epc-net-l"])
@pytest.mark.parametrize("n,B,P,Nn", [pytest.param(4096, 1, 2, 14, id="18x4096"), pytest.param(256, 2, 2, 4, id="2x8x256"),
                                      pytest.param(256, 1, 2, 6, id="10x256")])
def test_step_ids_is_the_same_step(dev, arch, prec, graph, n, B, P, Nn):
    """TrainStep.step_ids against TrainStep.step from equal initial state: loss, every updated variable, Adam moments and moving
    averages bit-equal after three steps with a different tuple each step (schedules change too: epoch 0 / 5 / 10, DECAY_STEP 2)."""
    M = 24
    data = torch.from_numpy(np.concatenate([O.synthetic_clouds(M - 4, n, 21, "lidar" if n == 4096 else "uniform"),
                                            O.synthetic_clouds(2, n, 22, "zeropad25"), O.synthetic_clouds(2, n, 23, "dup")], 0)).to(dev)
    tuples = _tuples(M, B, P, Nn)
    assert sum(int((np.concatenate(a, 1) != np.concatenate(b, 1)).sum()) for a, b in [(tuples[1], tuples[2])]) == 1
    ref = _run_steps(dev, arch, prec, B, graph, data, tuples, use_ids=False)
    got = _run_steps(dev, arch, prec, B, graph, data, tuples, use_ids=True)
    _assert_same_run(ref, got, (arch, prec, graph, n, B))


def test_distill_step_ids_is_the_same_step(dev):
    """DistillStep inherits step_ids: teacher and student both take the assembled clouds and graph (their point features follow the
    same Hilbert order either way), so the distillation step on ids is the distillation step on the clouds."""
    KD, V, ops = H.pkg("kd_training"), H.pkg("variables"), H.pkg("ops")
    n, M = 256, 16
    data = torch.from_numpy(O.synthetic_clouds(M, n, 31)).to(dev)
    params = dict(H.PARAMS, BATCH_NUM_QUERIES=1, ARCH_TEACHER="kd_epc-net", ARCH_STUDENT="kd_epc-net-l", GAMMA=0.5, ALPHA=0.1,
                  BASE_LEARNING_RATE=1e-3)
    tuples = _tuples(M, 1, 2, 4)
    runs = []
    for use_ids in (False, True):
        st = V.reset_default_store(device=dev, seed=0)
        ds = KD.DistillStep(params, st)
        with V.variable_scope(ds.teacher_outer):
            ds.teacher.declare_variables(params, n)
        ds._ensure_built(n)
        st.randomize_statistics(0)
        bank = None
        if use_ids:
            bank = ops.CloudBank(n, M, dev)
            bank.add(data)
        losses = []
        for i, tup in enumerate(tuples):
            if use_ids:
                loss, _, _ = ds.step_ids(bank, *tup, epoch=i)
            else:
                loss, _, _ = ds.step(*(data[torch.from_numpy(np.ascontiguousarray(x)).to(dev).long()] for x in tup), epoch=i)
            losses.append(float(loss))
        runs.append((losses, {k: v.detach().cpu().numpy().copy() for k, v in st.vars.items()}))
    _assert_same_run(runs[0], runs[1], "distill")


def test_bad_ids_and_refused_records(dev):
    """An id outside the bank: no fault, NaN coordinates in that slot (a non-finite loss), check() raises and names the slot, and the
    next valid step equals the step of a run that never saw the bad id.  A record that does not fit 16 bits is refused with a
    status -- n > 65536 by the entry point, a forged index by the store's first pass -- and nothing is stored."""
    ops, L, TR = H.pkg("ops"), H.pkg("lib"), H.pkg("training")
    lib = L.lib()
    n, M = 256, 12
    data = torch.from_numpy(O.synthetic_clouds(M, n, 41)).to(dev)
    bank = ops.CloudBank(n, M, dev)
    bank.add(data)
    # -- assemble with ids outside [0, M): slots 1, 3 (negative) and 35 (the second status word)
    ids = torch.arange(40, dtype=torch.int32, device=dev) % M
    ids[1], ids[3], ids[35] = M, -1, 1 << 20
    out = bank.buffers(40)
    out["idx"].fill_(0x7fffffff)                       # stale garbage no consumer may follow
    xyz, g = bank.assemble(ids, out=out)
    good = torch.ones(40, dtype=torch.bool, device=dev)
    good[[1, 3, 35]] = False
    assert torch.isnan(xyz[~good]).all() and torch.isfinite(xyz[good]).all()
    assert torch.isnan(out["poison"]).all()            # this launch's verdict, for the step's loss (0 when every id is inside)
    assert int(g.cnt[~good].abs().max()) == 0 and int(g.idx[~good].abs().max()) == 0
    assert int(g.transposed()[0].view(40, n)[~good].abs().max()) == 0 and int(g.overflow()[0][~good].abs().max()) == 0
    ids_ok = ids.clone()
    ids_ok[~good] = 0
    want = _fresh(data[ids_ok.long()])
    assert torch.equal(xyz[good], want["xyz"][good]) and torch.equal(g.cnt[good], want["cnt"][good])
    with pytest.raises(L.EpcNetError, match=r"\[1, 3, 35\]"):
        bank.check()
    bank.check()                                       # (cleared by the raising check)
    bank.assemble(ids_ok, out=out)
    assert float(out["poison"]) == 0.0
    bank.check()
    # -- a step with a bad id, then a valid one
    tuples = _tuples(M, 1, 2, 4, steps=2)
    bad = tuple(x.copy() for x in tuples[0])
    bad[2][0, 1] = M + 7                               # slot 1 + 2 + 1 = 4 of the tuple
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=1, TRAIN_PRECISION="bf16x6", BASE_LEARNING_RATE=1e-3)
    res = []
    for with_bad in (False, True):
        st = H.make_store("epc-net-l", O.seeded_weights("epc-net-l", 4), dev)
        ts = TR.TrainStep(params, st, outer=H.OUTER)
        if with_bad:
            snap = {k: v.detach().clone() for k, v in st.vars.items()}
            loss, _, _ = ts.step_ids(bank, *bad)
            assert not np.isfinite(float(loss))
            with pytest.raises(L.EpcNetError, match=r"slot\(s\) \[4\]"):
                bank.check()
            # (what a caller does after a poisoned step: back to the last good state -- here the initial one)
            with torch.no_grad():
                for k, v in st.vars.items():
                    v.copy_(snap[k])
            for d in (ts.m, ts.v):
                for v in d.values():
                    v.zero_()
            ts.global_step = 0
        loss, _, _ = ts.step_ids(bank, *tuples[1])
        bank.check()
        res.append(([float(loss)], {k: v.detach().cpu().numpy().copy() for k, v in st.vars.items()}))
    assert np.isfinite(res[0][0][0]) and res[0][0] == res[1][0]
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    # -- records that do not fit
    assert lib.epc_bank_record_bytes(65536 + 8, CAP) == 0 and lib.epc_bank_record_bytes(4100, CAP) == 0
    assert lib.epc_bank_record_bytes(4096, CAP) == 16 + 4096 * 158 and lib.epc_bank_record_bytes(65536, CAP) > 0
    EINVAL = -1                                                      # include/epcnet.h: EPC_EINVAL
    f = _fresh(data[:2])
    before = bank.records.clone()
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def store(n_arg, t, first=0):
        return lib.epc_bank_store(bank.records.data_ptr(), M, first, 2, n_arg, CAP, t["xyz"].data_ptr(), t["kth"].data_ptr(),
                                  t["cnt"].data_ptr(), t["idx"].data_ptr(), t["rdeg"].data_ptr(), t["roff"].data_ptr(),
                                  t["rlist"].data_ptr(), t["ovf_cnt"].data_ptr(), t["ovf_list"].data_ptr(), status.data_ptr(),
                                  L.current_stream())
    assert store(65536 + 8, f) == EINVAL                       # n > 65536: refused by the entry point
    assert store(n, f, first=M - 1) == EINVAL                  # slots outside the bank
    for name, where, value in (("idx", (1, 5, 0), 70000), ("idx", (0, 9, 3), -1), ("rlist", (n * CAP + 2,), n * 2 + 70000),
                               ("rlist", (0,), n + 1), ("ovf_cnt", (1,), n + 1), ("roff", (7,), 65536 * 3)):
        forged = {k: v.clone() for k, v in f.items()}
        assert int(f["cnt"][1, 5]) > 0 and int(f["cnt"][0, 9]) > 3 and int(f["rdeg"].view(2, n)[1].sum()) > 2
        forged[name][where] = value
        status.zero_()
        assert store(n, forged) == L.EPC_OK
        assert int(status.item()) != 0, (name, where)                # refused by the first pass ...
        assert torch.equal(bank.records, before), (name, where)      # ... and nothing was stored
    status.zero_()
    assert store(n, f) == L.EPC_OK and int(status.item()) == 0       # the unforged batch is accepted (records 0, 1 rewritten alike)
    assert torch.equal(bank.records, before)
    with pytest.raises(L.EpcNetError):
        bank.add(data[:1])                                           # full
    with pytest.raises(L.EpcNetError):
        bank.assemble(torch.zeros(4, dtype=torch.int32))             # CPU ids: no CPU fallback
    with pytest.raises(L.EpcNetError):
        ops.CloudBank(n, 4, dev).add(data[:1].cpu())


def _dataset(T, n, seed=0):
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1, 1, (T, n, 3)).astype(np.float32)
    queries = {}
    for i in range(T):
        queries[i] = {"query": "%d.bin" % i, "positives": [j for j in range(T) if j != i and abs(j - i) <= 2],
                      "negatives": [j for j in range(T) if abs(j - i) > 4]}
    return queries, data


class _Keep(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize("nq", [1, 2])
def test_trainer_on_the_bank_is_the_same_run(dev, tmp_path, nq):
    """Trainer(bank=True) against Trainer(bank=False) with the same seeds of ``random`` / ``numpy``, on the synthetic dataset of
    tests/test_gpu_kd_and_loop.py: the same loss sequence (equal floats), the same skip messages and the same checkpoint tensors over
    an epoch slice that crosses a mining refresh (epoch > 5, i % (1400 // B) == 29 -> 31 iterations), eager then replayed, then a save,
    a resume in a fresh store and two more iterations.  Query 5 has fewer than P positives: the "FAULTY TUPLE" skip (the "NO OTHER NEG"
    skip: test_no_other_neg_skip_is_the_same)."""
    V, TR, TL = H.pkg("variables"), H.pkg("training"), H.pkg("train_loop")
    N, T = 128, 40
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=nq, POSITIVES_PER_QUERY=2, NEGATIVES_PER_QUERY=6,
                  NUM_POINTS=N, BASE_LEARNING_RATE=1e-3, MAX_EPOCH=8)
    runs = []
    for use_bank in (False, True):
        queries, data = _dataset(T, N)
        queries[5]["positives"] = [4]                          # fewer than P positives: "FAULTY TUPLE"
        st = V.reset_default_store(device=dev, seed=0)
        ts = TR.TrainStep(params, st)
        ts._ensure_built(N)
        st.randomize_statistics(0)
        log = logging.getLogger("bank-%d-%d" % (nq, use_bank))
        log.setLevel(logging.INFO)
        keep = _Keep()
        log.addHandler(keep)
        save = str(tmp_path / ("bank%d" % use_bank))
        tr = TL.Trainer(ts, queries, data, queries, data, save_path=save, logger=log, bank=use_bank)
        assert (tr.bank is not None) == use_bank
        np.random.seed(0)
        random.seed(0)
        tr.TRAINING_LATENT_VECTORS = tr.get_latent_vectors()    # the mining branch from the first iteration on
        losses = tr.train_one_epoch(6, max_iters=31 if nq == 1 else 16)      # crosses i == 29 (nq 1): the descriptor cache refresh
        tr.graph = True
        losses += tr.train_one_epoch(6, max_iters=4)
        tr.graph = False
        ev = tr.evaluate_loss(6)
        prefix = tr.save(6, 101)
        ckpt = tr.checkpoint_tensors()
        # resume in a fresh store, on the same kind of trainer, and continue
        st2 = V.reset_default_store(device=dev, seed=123)
        ts2 = TR.TrainStep(params, st2)
        tr2 = TL.Trainer(ts2, queries, data, save_path=save, logger=log, bank=use_bank)
        tr2.restore(prefix)
        tr2.TRAINING_LATENT_VECTORS = tr2.get_latent_vectors()
        losses += tr2.train_one_epoch(7, max_iters=2)
        ckpt2 = tr2.checkpoint_tensors()
        skips = [m.split("] ")[-1] for m in keep.lines if m.endswith("!!!")]
        refreshed = sum("Updated cached feature vectors" in m for m in keep.lines)
        if use_bank:
            assert any(m.startswith("Cloud bank: %d clouds" % T) for m in keep.lines)
        runs.append((losses, ev, ckpt, ckpt2, skips, refreshed, [m for m in keep.lines if "Loss" in m or m.endswith("!!!")]))
        log.removeHandler(keep)
    a, b = runs
    assert len(a[0]) >= 20 and all(np.isfinite(a[0]))
    assert a[0] == b[0]                                         # the loss sequence: equal floats
    assert a[1] == b[1]
    assert a[4] == b[4] and a[6] == b[6]                        # the same skips at the same iterations, the same log lines
    assert nq == 2 or a[5] >= 1                                 # the slice really crossed a refresh of the descriptor cache
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k


def test_no_other_neg_skip_is_the_same(dev):
    """A query dict in which one query has no possible other negative: both trainers log "NO OTHER NEG" for it and step alike."""
    V, TR, TL = H.pkg("variables"), H.pkg("training"), H.pkg("train_loop")
    N, T = 128, 12
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=1, POSITIVES_PER_QUERY=2, NEGATIVES_PER_QUERY=3, NUM_POINTS=N)
    runs = []
    for use_bank in (False, True):
        rng = np.random.default_rng(3)
        data = rng.uniform(-1, 1, (T, N, 3)).astype(np.float32)
        queries = {i: {"query": "%d.bin" % i, "positives": [j for j in range(T) if j != i and j % 2 == i % 2],
                       "negatives": [j for j in range(T) if j % 2 != i % 2]} for i in range(T)}
        queries[0]["positives"] = list(range(T))                # query 0: every cloud is its positive -> nothing is left over
        st = V.reset_default_store(device=dev, seed=0)
        ts = TR.TrainStep(params, st)
        ts._ensure_built(N)
        st.randomize_statistics(0)
        log = logging.getLogger("bank-noneg-%d" % use_bank)
        log.setLevel(logging.INFO)
        keep = _Keep()
        log.addHandler(keep)
        tr = TL.Trainer(ts, queries, data, logger=log, bank=use_bank)
        np.random.seed(1)
        random.seed(1)
        losses = tr.train_one_epoch(1)
        runs.append((losses, [m for m in keep.lines if m.endswith("!!!")]))
        log.removeHandler(keep)
    assert runs[0] == runs[1]
    # query 0 always skips; the five other even queries always step (their negatives are odd clouds, whose positives are the odd
    # clouds: the query itself is what is left over); an odd query skips when it draws cloud 0 as a negative
    assert any("NO OTHER NEG" in m for m in runs[0][1]) and len(runs[0][0]) >= 5


def test_replay_loop_on_ids_in_a_child_process():
    """40 replays of step_ids with alternating id sets, back to back without waiting for the stream -- across one REPLAYS_PER_SYNC
    boundary -- all losses finite and equal to the eager sequence.  In a child under its own time limit, run once (the pattern of
    tests/test_gpu_train_step.py::test_long_unsynchronised_replay_loop_in_a_child_process): a functional check, not a soak."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import helpers as H
from helpers import O
TR, ops = H.pkg("training"), H.pkg("ops")
assert 32 <= TR.REPLAYS_PER_SYNC < 40
dev = torch.device("cuda:0")
n, M = 4096, 30
data = torch.from_numpy(O.synthetic_clouds(M, n, 9)).to(dev)
bank = ops.CloudBank(n, M, dev)
bank.add(data)
rng = np.random.RandomState(5)
sets = [rng.permutation(M)[:18].reshape(1, 18) for _ in range(3)]
split = lambda f: (f[:, :1], f[:, 1:3], f[:, 3:17], f[:, 17:])
out = []
for graph in (False, True):
    st = H.make_store("epc-net", O.seeded_weights("epc-net", 4), dev)
    ts = TR.TrainStep(dict(H.PARAMS, ARCH="epc-net", BATCH_NUM_QUERIES=1, TRAIN_PRECISION="bf16"), st, outer=H.OUTER)
    losses = [ts.step_ids(bank, *split(sets[k %% 3]), epoch=0, graph=graph)[0] for k in range(40)]
    torch.cuda.synchronize()
    out.append([float(x) for x in losses])
bank.check()
ops.chain_persist_check()
assert all(np.isfinite(out[0])) and out[0] == out[1], (out[0][:4], out[1][:4])
print("CHILD OK", out[1][-1])
""" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])


def test_data_parallel_step_ids_in_a_child_process():
    """The data-parallel form -- eager around the two all-reduces, and replayed as THREE graphs with the assemble launch inside the
    first -- on a process group of one rank with the single-rank short-circuits switched off (the pattern of
    tests/test_gpu_rccl_world1.py; in a child: it owns its process group): step_ids == the plain single-process step, bit for bit
    (the mean over one rank is the identity)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, socket, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r); sys.path.insert(0, %r)
import helpers as H
from helpers import O
TR, ops, D = H.pkg("training"), H.pkg("ops"), H.pkg("distributed")
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
n, M = 256, 16
data = torch.from_numpy(O.synthetic_clouds(M, n, 9)).to(dev)
bank = ops.CloudBank(n, M, dev)
bank.add(data)
rng = np.random.RandomState(5)
sets = [rng.permutation(M)[:10].reshape(1, 10) for _ in range(3)]
split = lambda f: (f[:, :1], f[:, 1:3], f[:, 3:9], f[:, 9:])
params = dict(H.PARAMS, ARCH="epc-net", BATCH_NUM_QUERIES=1, TRAIN_PRECISION="bf16x6", BASE_LEARNING_RATE=1e-3)

def run(mode, graph):
    st = H.make_store("epc-net", O.seeded_weights("epc-net", 4), dev)
    ts = TR.TrainStep(params, st, outer=H.OUTER)
    losses = []
    for k in range(3):
        if mode == "ids":
            losses.append(float(ts.step_ids(bank, *split(sets[k]), epoch=k, graph=graph)[0]))
        else:
            losses.append(float(ts.step(*(data[torch.from_numpy(x).to(dev)] for x in split(sets[k])), epoch=k, graph=graph)[0]))
    torch.cuda.synchronize()
    if graph and D.collectives_active():          # the three-graph form, fed by the bank
        assert ts._graph["dp"] and "graph2" in ts._graph and ts._graph["source"] is not None
    return losses, {k: v.detach().cpu().numpy().copy() for k, v in st.vars.items()}

ref = run("clouds", False)                     # single process, no collectives
s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
D.force_collective(True)
assert D.collectives_active()
for graph in (False, True):
    got = run("ids", graph)
    assert all(np.isfinite(got[0])) and got[0] == ref[0], (graph, got[0], ref[0])
    for k in ref[1]:
        assert np.array_equal(ref[1][k], got[1][k]), (graph, k)
bank.check()
D.force_collective(False)
dist.barrier()
dist.destroy_process_group()
print("CHILD OK")
""" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
