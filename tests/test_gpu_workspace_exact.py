"""Workspaces of exactly the size the query names.  A size query and the launcher's carving of the buffer come from one layout function
(csrc/common.h: epc_carver); these tests are the other half of that contract -- every entry that takes a workspace, a scratch or a
partial buffer runs on one of EXACTLY the queried size between poisoned guards, and neither writes outside it nor computes anything else
than on a roomy one.

The training step never sees an exact buffer by itself: ops._ws, ops._splitk_ws and ops._scratch_bytes hand out cached buffers of at
least 1 MiB / 2^18 floats.  Here they are replaced, for one eager step, by providers of fresh Guarded buffers of the requested size filled
with 0xFF (a NaN pattern: a kernel that read a word before writing it would change the step's result, which is bit-reproducible)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from helpers import Guarded, O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


def _step(arch, precision, n, dev):
    """One eager training step on 1 query of 18 clouds x n points from seeded weights -> (loss, {variable: value})."""
    TR = H.pkg("training")
    nneg = 14
    pcs = torch.from_numpy(O.synthetic_clouds(18, n, 9)).to(dev)
    q, pos, neg, oth = pcs[None, :1], pcs[None, 1:3], pcs[None, 3:3 + nneg], pcs[None, 3 + nneg:]
    params = dict(H.PARAMS, ARCH=arch, BATCH_NUM_QUERIES=1, DECAY_STEP=200000, BASE_LEARNING_RATE=5e-5, MARGIN_1=0.5, MARGIN_2=0.2,
                  TRAIN_PRECISION=precision)
    st = H.make_store(arch, O.seeded_weights(arch, 4), dev)
    ts = TR.TrainStep(params, st, outer=H.OUTER)
    loss, _, _ = ts.step(q, pos, neg, oth, epoch=0)
    torch.cuda.synchronize()
    return float(loss), {k: v.detach().cpu().numpy().copy() for k, v in st.vars.items()}


# n = 256: the streamed head on whole 128-row tiles; n = 96: every per-cloud 128-row tile partial, the 96-row grid of the shared-operand
# assignment divides evenly (18 tiles); n = 48: the per-layer operators -- column reductions, partial buffers, split-K products
STEP_CASES = [("epc-net", 256), ("epc-net", 96), ("epc-net", 48), ("epc-net-l", 256)]


@pytest.mark.parametrize("precision", ["bf16x6", "bf16"])
@pytest.mark.parametrize("arch,n", STEP_CASES, ids=["%s-18x%d" % c for c in STEP_CASES])
def test_training_step_on_exact_size_workspaces(dev, monkeypatch, arch, n, precision):
    ops, L = H.pkg("ops"), H.pkg("lib")
    if arch == "epc-net":
        assert (ops.head_stream_mode(18 * n, 256, 1024, n) is None) == (n == 48)
    want_loss, want = _step(arch, precision, n, dev)
    handed = []                                      # every buffer stays alive (and its guards readable) until the step has finished

    def exact(count, dtype, device):
        g = Guarded((int(count),), dtype, device)
        handed.append(g)
        return g.t

    def ws(rows, C, device):
        need = L.lib().epc_colreduce_workspace_bytes(int(rows), int(C))
        return exact(need, torch.uint8, device), need

    monkeypatch.setattr(ops, "_ws", ws)
    monkeypatch.setattr(ops, "_splitk_ws", lambda floats, device: exact(floats, torch.float32, device))
    monkeypatch.setattr(ops, "_scratch_bytes", lambda nbytes, device: (exact(nbytes, torch.uint8, device), int(nbytes)))
    got_loss, got = _step(arch, precision, n, dev)
    monkeypatch.undo()
    kinds = {str(g.t.dtype) for g in handed}
    print("%s %s 18x%d: %d exact buffers (%s), %d bytes in all, loss %.9g" % (arch, precision, n, len(handed), ", ".join(sorted(kinds)),
                                                                              sum(g.nbytes for g in handed), got_loss))
    assert len(kinds) == 2, "the step asked for no column-reduction / scratch buffer, or for no partial buffer"
    broken = [i for i, g in enumerate(handed) if not g.intact()]
    assert not broken, "a write outside %d of %d exact-size buffers (in the order handed out: %s)" % (len(broken), len(handed), broken[:8])
    assert np.isfinite(want_loss) and got_loss == want_loss
    assert set(got) == set(want)
    for k, v in want.items():
        assert np.array_equal(v, got[k]), k


def _twice(call, need, outs, dev):
    """call(workspace tensor, its bytes) on a Guarded workspace of exactly `need` bytes and on one 4096 bytes larger; `outs()` makes the
    Guarded outputs of one call.  Guards intact, outputs bit-equal -> the outputs of the exact call."""
    results = []
    for extra in (0, 4096):
        ws, o = Guarded((need + extra,), torch.uint8, dev), outs()
        call(ws.t, need + extra, *[g.t for g in o])
        torch.cuda.synchronize()
        assert ws.intact() and all(g.intact() for g in o), "a write outside a buffer (workspace of the queried size + %d)" % extra
        assert not any(g.untouched() for g in o)
        results.append([g.t.clone() for g in o])
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return results[0]


def test_pairwise_topk_on_an_exact_workspace(dev):
    """300 database rows x 130 queries, dim 8, k 5: three database tiles of 128 with the last partial, two query tiles."""
    L = H.pkg("lib")
    nd, nq, dim, k = 300, 130, 8, 5
    g = torch.Generator().manual_seed(11)
    db, q = torch.randn((nd, dim), generator=g).to(dev), torch.randn((nq, dim), generator=g).to(dev)
    need = L.lib().epc_pairwise_topk_workspace_bytes(nd, nq)
    assert need > 0
    idx, dist = _twice(lambda ws, n, idx, dist: L.run.epc_pairwise_topk_ws(db, nd, q, nq, dim, k, idx, dist, ws, n), need,
                       lambda: [Guarded((nq, k), torch.int32, dev), Guarded((nq, k), torch.float32, dev)], dev)
    d = torch.cdist(q.double(), db.double())
    ref = torch.sort(d, dim=1).values[:, :k]
    assert (dist.double() - ref).abs().max() <= 1e-5 and bool((idx >= 0).all()) and bool((idx < nd).all())


def test_mine_topk_on_an_exact_workspace(dev):
    """3 queries, max_cand 70 (two slabs of 64 candidates), k 5."""
    L = H.pkg("lib")
    rows, dim, nq, max_cand, k = 200, 8, 3, 70, 5
    g = torch.Generator().manual_seed(12)
    table, q = torch.randn((rows, dim), generator=g).to(dev), torch.randn((nq, dim), generator=g).to(dev)
    cand = torch.stack([torch.randperm(rows, generator=g)[:max_cand] for _ in range(nq)]).to(torch.int32).to(dev)
    count = torch.tensor([70, 65, 9], dtype=torch.int32, device=dev)
    need = L.lib().epc_mine_topk_workspace_bytes(nq, max_cand)
    assert need > 0
    pos, ids, dist = _twice(lambda ws, n, pos, ids, dist: L.run.epc_mine_topk(table, rows, dim, q, nq, cand, count, max_cand, k, pos, ids,
                                                                               dist, ws, n), need,
                            lambda: [Guarded((nq, k), torch.int32, dev), Guarded((nq, k), torch.int32, dev),
                                     Guarded((nq, k), torch.float32, dev)], dev)
    for i in range(nq):
        c = cand[i, :int(count[i])].long()
        d = torch.cdist(q[i:i + 1].double(), table[c].double())[0]
        order = torch.sort(d).indices[:k]
        assert (dist[i].double() - d[order]).abs().max() <= 1e-5
        assert torch.equal(ids[i].long(), c[pos[i].long()])


def test_vlad_head_on_an_exact_workspace(dev):
    """3 clouds, GROUPS 4: the call form of helpers.run_stages."""
    L = H.pkg("lib")
    lib = L.lib()
    nc = 3
    eng, _ = H.make_engine("epc-net", O.seeded_weights("epc-net", 0), dev)
    cfg = eng.cfg_for(256)
    assert cfg.groups == 4
    packed = eng.packed(cfg)
    head = packed.data_ptr() + lib.epc_net_packed_offset(ctypes.byref(cfg), 6)
    g = torch.Generator().manual_seed(13)
    V = torch.randn((nc, 1024, 64), generator=g).to(dev)
    colss = (V.reshape(nc, 32, 32, 64) ** 2).sum(dim=2).contiguous()
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    need = lib.epc_vlad_head_workspace_bytes(nc, cfg.groups)
    assert need > 0
    desc, = _twice(lambda ws, n, desc: L.run.epc_vlad_head_fwd(V, colss, head, cfg.groups, nc, desc, status, ws, n), need,
                   lambda: [Guarded((nc, 256), torch.float32, dev)], dev)
    assert bool(torch.isfinite(desc).all()) and (desc.double().norm(dim=1) - 1.0).abs().max() <= 1e-5
