"""GPU tests of the PERSISTENT forward of the backbone chain (csrc/train_chain_persist.hip: one launch, grid-wide barriers instead of
kernel boundaries; models/epc-net.py:66-134 in training mode) against the launch chain it replaces (csrc/train_chain.hip) -- the same
products in the same arithmetic on the same operands; only the summation order of the batch statistics differs (group partials by row
range instead of sixteen strided slices) -- and of the two things the kernel's header rests on beyond that comparison: its coherence
rule under reuse of the same buffers (the soaks) and what an abandoned launch does to a training step (the loss must say so)."""
import logging
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O
from test_gpu_chain import _backbone, hold_to_the_per_layer_operators

pytestmark = pytest.mark.gpu
ERR_WORD = 2112          # the workspace's sticky error word as an int32 index (PST_W_ERR of csrc/train_chain_persist.hip)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _with_persist(on, fn):
    ops = H.pkg("ops")
    prev = ops.CHAIN_PERSIST_FWD
    ops.CHAIN_PERSIST_FWD = on
    try:
        out = fn()
        ops.chain_persist_check()
        return out
    finally:
        ops.CHAIN_PERSIST_FWD = prev


def test_first_launch_in_a_child_process():
    """The very first persistent launches of a session run in a CHILD with a hard time limit: a grid barrier that could not complete
    (a workgroup not resident) must end in the kernel's own bounded spin and an EPC_EHIP, never in a hung device."""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import helpers as H
from helpers import O
from test_gpu_chain import _backbone
ops = H.pkg("ops")
dev = torch.device("cuda:0")
assert H.pkg("lib").lib().epc_chain_persist_ok(4 * 256) == 1
w = O.seeded_weights("epc-net", 4); pc = O.synthetic_clouds(4, 256, 5)
ops.CHAIN_PERSIST_FWD = True
a = _backbone("epc-net", w, pc, dev, True)
ops.chain_persist_check()
ops.CHAIN_PERSIST_FWD = False
b = _backbone("epc-net", w, pc, dev, True)
print("max diff", float(np.abs(a[0] - b[0]).max()))
assert np.isfinite(a[0]).all() and np.abs(a[0] - b[0]).max() <= 1e-5 * max(np.abs(b[0]).max(), 1.0)
print("CHILD OK")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("arch,ncl,n,kind,precision", [("epc-net", 3, 256, "uniform", "bf16x6"), ("epc-net-l", 5, 96, "uniform", "bf16x6"),
                                                      ("epc-net", 2, 32, "uniform", "bf16x6"),          # two workgroups of one wave: two groups of one
                                                      ("epc-net", 2, 256, "ties", "bf16x6"), ("epc-net", 18, 4096, "uniform", "bf16x6"),
                                                      ("epc-net", 22, 4096, "uniform", "bf16"), ("epc-net", 7, 1000, "uniform", "bf16"),
                                                      ("epc-net", 24, 4096, "uniform", "bf16x6")])      # twelve waves: the largest form
def test_persistent_chain_equals_the_launch_chain(dev, arch, ncl, n, kind, precision):
    """Outputs to 1e-5 of their scale, moving statistics to 2e-6, gradients to 1e-4 relative L2 (small sizes; at full size ReLU-mask
    flips between two float32 summation orders move single gradient elements: the bars of test_gpu_chain)."""
    lib = H.pkg("lib").lib()
    assert lib.epc_chain_persist_ok(ncl * n) == 1
    if ncl * n == 24 * 4096:       # 256 workgroups of twelve 32-row tiles (waves) on 256 CUs: the persistent kernel's largest LDS
        parts = lib.epc_chain_parts(ncl * n)
        assert (parts, -(-ncl * n // parts) // 32) == (256, 12), (parts, torch.cuda.get_device_properties(0).multi_processor_count)
    w = O.seeded_weights(arch, 4)
    pc = O.synthetic_clouds(ncl, n, 11)
    if kind == "ties":
        pc[0, 40:120] = pc[0, 7]
        pc[1] = 0.0
    a = _with_persist(True, lambda: _backbone(arch, w, pc, dev, True, precision=precision))
    b = _with_persist(False, lambda: _backbone(arch, w, pc, dev, True, precision=precision))
    assert np.isfinite(a[0]).all()
    small = n < 4096 and kind == "uniform"
    bar_out, bar_grad = (1e-5, 1e-4) if small else ((5e-5, 2e-2) if kind == "uniform" else (1e-4, 2e-2))
    if precision == "bf16":
        # One bf16 value per operand: the last bit of a batch moment moves rounding boundaries of the operands it normalises, so two
        # correct implementations of this arithmetic differ by single bf16 ulps of single elements (2^-9 of an element, grown through
        # twelve layers).  What is held instead: the two lie equally far from the f32-accurate chain (a systematic error would show
        # there) and much closer to each other than to it.
        c = _with_persist(False, lambda: _backbone(arch, w, pc, dev, True, precision="bf16x6"))
        rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
        dab, dac, dbc = rel(a[0], b[0]), rel(a[0], c[0]), rel(b[0], c[0])
        print("bf16: persistent vs launch %.2e; vs the f32-accurate chain: persistent %.2e, launch %.2e" % (dab, dac, dbc))
        assert abs(dac - dbc) <= 0.1 * dbc and dab <= 0.5 * dbc, (dab, dac, dbc)
        bar_out, bar_grad = 3e-2, 5e-2
    assert np.abs(a[0] - b[0]).max() <= bar_out * max(np.abs(b[0]).max(), 1.0)
    worst = (0.0, "")
    for k, gb in b[1].items():
        ga = a[1][k]
        if gb is None or k.endswith("/biases"):
            assert ga is None or np.abs(ga).max() <= 1e-4
            continue
        rel = np.linalg.norm(ga - gb) / max(np.linalg.norm(gb), 1e-30)
        if precision == "bf16":      # as the outputs: as far from the f32-accurate gradient as the launch chain's, closer to it than to that
            gc = c[1][k]
            rac, rbc = np.linalg.norm(ga - gc) / np.linalg.norm(gc), np.linalg.norm(gb - gc) / np.linalg.norm(gc)
            worst = max(worst, (rel / rbc, k))
            assert rac <= 1.3 * rbc + 1e-3 and rel <= 1.2 * rbc + 1e-3, (k, rel, rac, rbc)
            continue
        worst = max(worst, (rel, k))
        assert rel <= bar_grad, (k, rel)
    for k, vb in b[2].items():
        bar = (2e-6 if kind == "uniform" else 5e-5) if precision != "bf16" else 5e-3      # (bf16: the statistics of bf16-rounded products)
        assert np.abs(a[2][k] - vb).max() <= 2e-6 + bar * np.abs(vb).max(), k
    print("persistent vs launch chain, %s %dx%d (%s, %s): cat max diff %.2e, worst gradient rel L2 (bf16: / the launch chain's distance from f32) %.2e (%s)"
          % (arch, ncl, n, kind, precision, np.abs(a[0] - b[0]).max(), worst[0], worst[1]))


def test_persistent_chain_is_bit_reproducible(dev):
    w = O.seeded_weights("epc-net", 4)
    pc = O.synthetic_clouds(18, 4096, 5)
    a = _with_persist(True, lambda: _backbone("epc-net", w, pc, dev, True))
    b = _with_persist(True, lambda: _backbone("epc-net", w, pc, dev, True))
    assert np.array_equal(a[0], b[0])
    for k in a[1]:
        assert (a[1][k] is None and b[1][k] is None) or np.array_equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


def test_abandoned_barrier_is_reported_not_hung(dev):
    """A launch whose barrier cannot complete (here: a spin budget of ONE tick, so the first workgroup that has to wait gives up) sets
    the sticky error word, every workgroup leaves, epc_chain_persist_status returns EPC_EHIP, later launches return at once until the
    reset -- and after the reset the chain runs again and agrees with the launch chain."""
    L, ops = H.pkg("lib"), H.pkg("ops")
    lib = L.lib()
    w = O.seeded_weights("epc-net", 4)
    pc = O.synthetic_clouds(18, 4096, 5)
    ws = ops.chain_workspace(dev)
    words = ws.view(torch.int32)
    prev_ticks, prev_flags = ops.CHAIN_SPIN_TICKS, ops.CHAIN_PERSIST_FWD
    try:
        ops.CHAIN_PERSIST_FWD = True
        ops.CHAIN_SPIN_TICKS = 1
        _backbone("epc-net", w, pc, dev, True)
        torch.cuda.synchronize()
        assert lib.epc_chain_persist_status(ws.data_ptr(), L.current_stream()) == -3
        assert int(words[2112]) == 1
        seq = int(words[0])
        _backbone("epc-net", w, pc, dev, True)          # returns at once (results undefined), the word stays set
        assert lib.epc_chain_persist_status(ws.data_ptr(), L.current_stream()) == -3
        with pytest.raises(L.EpcNetError):
            ops.chain_persist_check()                    # raises and resets
        ops.CHAIN_SPIN_TICKS = prev_ticks
        torch.cuda.synchronize()
        assert int(words[2112]) == 0 and int(words[2048]) == 0 and int(words[0]) == seq + 1
        a = _backbone("epc-net", w, pc, dev, True)
        ops.chain_persist_check()
        ops.CHAIN_PERSIST_FWD = False
        b = _backbone("epc-net", w, pc, dev, True)
        assert np.isfinite(a[0]).all() and np.abs(a[0] - b[0]).max() <= 5e-5 * np.abs(b[0]).max()
    finally:
        ops.CHAIN_SPIN_TICKS = prev_ticks
        ops.CHAIN_PERSIST_FWD = prev_flags


def test_rows_beyond_the_persistent_form_take_the_launch_chain(dev):
    """More than twelve 32-row tiles per workgroup (25 x 4096 rows on 256 CUs: thirteen) is not covered: epc_chain_persist_ok says so and
    ProxyConvChain takes the launches -- same interface, no error."""
    lib = H.pkg("lib").lib()
    assert lib.epc_chain_persist_ok(24 * 4096) == 1 and lib.epc_chain_persist_ok(25 * 4096) == 0
    w = O.seeded_weights("epc-net-l", 4)
    pc = O.synthetic_clouds(25, 4096, 5)
    a = _with_persist(True, lambda: _backbone("epc-net-l", w, pc, dev, True))
    b = _with_persist(False, lambda: _backbone("epc-net-l", w, pc, dev, True))
    assert np.array_equal(a[0], b[0])
    # (both settings took the launch chain, so the comparison above only shows that no persistent launch happened: the result is also
    # held to the per-layer operators with test_gpu_chain's bars)
    c = _backbone("epc-net-l", w, pc, dev, False)
    hold_to_the_per_layer_operators(a, c, "epc-net-l", 25, 4096, "uniform")


# ---- soaks of the coherence rule -----------------------------------------------------------------------------------------------------
# The kernel's header: whatever another workgroup reads inside the launch is written exactly once per launch before its first read, a
# launch starts with L1 and L2 invalidated (so readers use plain loads), and a granule an earlier launch left in the workspace carries
# an older sequence number.  A stale line or a stale granule shows only when the SAME buffers come back with other contents, or when a
# smaller grid follows a larger one whose partial slots stay behind -- so: many launches in a row on recycled and on static buffers,
# every result held to the bits of the first result for the same input, and that first result held to the launch chain.

class _Forward:
    """The training-mode backbone forward alone, on ONE store: morton_sort -> KnnGraph -> tf_util.proxyconv_backbone under no_grad, no
    backward, no copy to the host.  Returns (cat, the 6 x nblocks batch moments stacked in layer order, the concat's bf16 copy or None),
    all on the device.  The moving-average updates are deferred and dropped, so the store never changes: the batch moments are what
    they would have consumed."""

    def __init__(self, arch, dev):
        self.nb = 4 if arch == "epc-net" else 2
        self.st = H.make_store(arch, O.seeded_weights(arch, 4), dev)

    def __call__(self, pc, precision="bf16x6", head_follows=False):
        V, tf_util, ops = H.pkg("variables"), H.pkg("utils.tf_util"), H.pkg("ops")
        prev = ops.set_gemm_precision(precision)
        tf_util.defer_ema_updates()
        try:
            with torch.no_grad(), V.variable_scope(H.OUTER), V.variable_scope("fastdgcnn"):
                x = ops.morton_sort(pc)
                cat = tf_util.proxyconv_backbone(x, ops.KnnGraph(x), 20, self.nb, bn_decay=0.7, is_training=True, head_follows=head_follows)
                moments = torch.stack([p[1] for p in tf_util._deferred_ema])
        finally:
            tf_util._deferred_ema = None
            tf_util.BACKBONE_TAP = None
            ops.set_gemm_precision(prev)
        assert tuple(moments.shape) == (6 * self.nb, 64)
        return cat, moments, getattr(cat, "_epc_bf16", None)


def _same(a, b):
    """All of a == b as a 0-d bool ON THE DEVICE: the soaks read their verdicts once at the end, so launches follow each other without
    a host round trip in between."""
    return (a == b).all()


def _same_result(a, b):
    ok = _same(a[0], b[0]) & _same(a[1], b[1])
    return ok & _same(a[2], b[2]) if a[2] is not None else ok


def _clouds(dev, ncl, n, seed, ties=False):
    pc = O.synthetic_clouds(ncl, n, seed)
    if ties:                                      # as test_persistent_chain_equals_the_launch_chain's "ties"
        pc[0, 40:120] = pc[0, 7]
        pc[1] = 0.0
    return torch.from_numpy(pc).to(dev)


def _hold_to_the_launch_chain(name, a, b, bar_out, bar_stat):
    """A persistent result against the launch chain's at test_persistent_chain_equals_the_launch_chain's bars: cat to bar_out of its
    scale; the batch moments to that test's bar on the moving statistics (2e-6 + bar_stat of the largest), which there is applied after
    shadow -= (1 - 0.7) (shadow - moment) from equal shadows -- the same bar on the moment itself is that bar / 0.3."""
    cat_a, cat_b = a[0].cpu().numpy(), b[0].cpu().numpy()
    diff, scale = float(np.abs(cat_a - cat_b).max()), max(float(np.abs(cat_b).max()), 1.0)
    ma, mb = a[1].cpu().numpy(), b[1].cpu().numpy()
    worst = float((np.abs(ma - mb).max(1) / ((2e-6 + bar_stat * np.abs(mb).max(1)) / 0.3)).max())
    print("%s: persistent vs launch chain: cat max diff %.2e, bar %.2e (%.0e of the scale %.2e); batch moments at %.2f of their bar"
          % (name, diff, bar_out * scale, bar_out, scale, worst))
    assert np.isfinite(cat_a).all() and diff <= bar_out * scale, (name, diff, scale)
    assert worst <= 1.0, (name, worst)


def _sequence_number(dev):
    torch.cuda.synchronize()
    return int(H.pkg("ops").chain_workspace(dev).view(torch.int32)[0])


def test_soak_alternating_shapes_eager(dev):
    """300 persistent launches in a row over five inputs of four shapes -- 2 to 24 workgroups, one of them twice with other contents,
    the tie clouds -- on buffers the allocator recycles: every cat and every batch moment is the same BITS as at the input's first
    occurrence; a reset in mid-soak (the sequence number advances) changes nothing; each first occurrence agrees with the launch chain."""
    L, ops = H.pkg("lib"), H.pkg("ops")
    lib = L.lib()
    fwd = _Forward("epc-net", dev)
    inputs = [("3x256", _clouds(dev, 3, 256, 11), False), ("7x1000", _clouds(dev, 7, 1000, 11), False), ("2x32", _clouds(dev, 2, 32, 11), False),
              ("3x256, other contents", _clouds(dev, 3, 256, 12), False), ("2x256 ties", _clouds(dev, 2, 256, 11, ties=True), True)]
    for _, pc, _ in inputs:
        assert lib.epc_chain_persist_ok(pc.shape[0] * pc.shape[1]) == 1      # (no member of the cycle quietly takes the launch chain)
    rounds = 60
    prev = ops.CHAIN_PERSIST_FWD
    try:
        ops.CHAIN_PERSIST_FWD = True
        ws = ops.chain_workspace(dev)
        seq0 = _sequence_number(dev)
        first, flags = {}, []
        for rnd in range(rounds):
            if rnd == rounds // 2:
                L.check(lib.epc_chain_persist_reset(ws.data_ptr(), L.current_stream()))
            for name, pc, _ in inputs:
                got = fwd(pc)
                if rnd == 0:
                    first[name] = got
                else:
                    flags.append(_same_result(got, first[name]))
        ok = torch.stack(flags).cpu().numpy().reshape(rounds - 1, len(inputs))
        # every call was a persistent launch that ran to its end (the last workgroup out advances the sequence number), + the reset
        assert _sequence_number(dev) - seq0 == rounds * len(inputs) + 1
        ops.chain_persist_check()
        assert ok.all(), "(round, input) whose bits differ from the input's first occurrence: %s" % (np.argwhere(~ok) + [1, 0]).tolist()[:20]
        ops.CHAIN_PERSIST_FWD = False
        for name, pc, ties in inputs:
            _hold_to_the_launch_chain(name, first[name], fwd(pc), *((1e-4, 5e-5) if ties else (1e-5, 2e-6)))
        assert _sequence_number(dev) - seq0 == rounds * len(inputs) + 1      # (those were launch chains)
    finally:
        ops.CHAIN_PERSIST_FWD = prev


@pytest.mark.parametrize("precision", ["bf16x6", "bf16"])
def test_soak_alternating_sizes_full(dev, precision):
    """18 x 4096 and 22 x 4096 in turn, 20 launches each: a workgroup holds 9 and 11 tiles, and the partial slots and group partials of
    the larger grid stay behind for the smaller one.  In both arithmetics; in bf16 the concat's bf16 copy (what the streamed head reads)
    is held too, to the bits of its first occurrence and to the f32 concat rounded to nearest even."""
    L, ops = H.pkg("lib"), H.pkg("ops")
    lib = L.lib()
    fwd = _Forward("epc-net", dev)
    inputs = [("18x4096", _clouds(dev, 18, 4096, 11)), ("22x4096", _clouds(dev, 22, 4096, 12))]
    tiles = []
    for _, pc in inputs:
        rows = pc.shape[0] * pc.shape[1]
        assert lib.epc_chain_persist_ok(rows) == 1
        tiles.append(-(-rows // lib.epc_chain_parts(rows)) // 32)
    assert tiles[0] < tiles[1] <= 12, tiles
    run = lambda pc, prec=precision: fwd(pc, prec, head_follows=(prec == "bf16"))
    each = 20
    prev = ops.CHAIN_PERSIST_FWD
    try:
        ops.CHAIN_PERSIST_FWD = True
        seq0 = _sequence_number(dev)
        first, flags = {}, []
        for rnd in range(each):
            for name, pc in inputs:
                got = run(pc)
                if rnd == 0:
                    first[name] = got
                else:
                    flags.append(_same_result(got, first[name]))
        ok = torch.stack(flags).cpu().numpy().reshape(each - 1, len(inputs))
        assert _sequence_number(dev) - seq0 == each * len(inputs)
        ops.chain_persist_check()
        assert ok.all(), "(round, input) whose bits differ from the input's first occurrence: %s" % (np.argwhere(~ok) + [1, 0]).tolist()[:20]
        ops.CHAIN_PERSIST_FWD = False
        for name, pc in inputs:
            a, b = first[name], run(pc)
            if precision == "bf16x6":
                _hold_to_the_launch_chain(name, a, b, 5e-5, 2e-6)
                assert a[2] is None
                continue
            # bf16: as test_persistent_chain_equals_the_launch_chain holds this arithmetic -- the two forms lie equally far from the
            # f32-accurate chain and much closer to each other than to it
            assert a[2] is not None and a[2].dtype == torch.bfloat16
            assert torch.equal(a[2], a[0].reshape(a[2].shape).to(torch.bfloat16)), "%s: the bf16 copy is not the f32 concat rounded to nearest even" % name
            c = run(pc, "bf16x6")
            rel = lambda x, y: float(torch.linalg.vector_norm((x - y).double()) / torch.linalg.vector_norm(y.double()))
            dab, dac, dbc = rel(a[0], b[0]), rel(a[0], c[0]), rel(b[0], c[0])
            print("%s bf16: persistent vs launch %.2e; vs the f32-accurate chain: persistent %.2e, launch %.2e" % (name, dab, dac, dbc))
            assert bool(torch.isfinite(a[0]).all()) and abs(dac - dbc) <= 0.1 * dbc and dab <= 0.5 * dbc, (name, dab, dac, dbc)
            assert float((a[0] - b[0]).abs().max()) <= 3e-2 * max(float(b[0].abs().max()), 1.0)
            assert float((a[1] - b[1]).abs().max()) <= 2e-6 + 5e-3 * float(b[1].abs().max()) / 0.3
    finally:
        ops.CHAIN_PERSIST_FWD = prev


@pytest.mark.parametrize("ncl,n,replays", [(3, 256, 150), (18, 4096, 40)])
def test_soak_graph_replay_static_buffers(dev, ncl, n, replays):
    """The form training runs: the forward captured ONCE into a HIP graph over a static cloud buffer -- every tensor of every replay at
    the same address -- and replayed with three contents in turn (A, B, and A with one cloud replaced: most rows' inputs unchanged).
    Every replay's cat and batch moments are the bits of the eager result for that content."""
    TR, ops = H.pkg("training"), H.pkg("ops")
    assert H.pkg("lib").lib().epc_chain_persist_ok(ncl * n) == 1
    fwd = _Forward("epc-net", dev)
    A, B = _clouds(dev, ncl, n, 11), _clouds(dev, ncl, n, 12)
    C = A.clone()
    C[1] = B[1]
    contents = [A, B, C]
    prev = ops.CHAIN_PERSIST_FWD
    try:
        ops.CHAIN_PERSIST_FWD = True
        ref = [fwd(pc) for pc in contents]          # eager: also the warm-up (the chain's workspace must exist before a capture)
        assert not _same(ref[0][0], ref[2][0]).item() and not _same(ref[0][0], ref[1][0]).item()
        static = A.clone()
        seq0 = _sequence_number(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):               # (captures on a side stream)
            out = fwd(static)
        assert _sequence_number(dev) == seq0        # (a capture runs nothing)
        order = [0, 0, 1, 1, 2, 2, 0, 2, 1]         # cycled: each content follows each content, itself included
        flags = []
        for i in range(replays):
            k = order[i % len(order)]
            static.copy_(contents[k])
            graph.replay()
            flags.append(_same_result(out, ref[k]))
            if (i + 1) % min(16, TR.REPLAYS_PER_SYNC) == 0:
                torch.cuda.current_stream().synchronize()
        ok = torch.stack(flags).cpu().numpy()
        assert _sequence_number(dev) - seq0 == replays      # every replay was a persistent launch that ran to its end
        ops.chain_persist_check()
        assert ok.all(), "replays (content) whose bits differ from the eager result: %s" % [(i, order[i % len(order)]) for i in np.flatnonzero(~ok)][:20]
    finally:
        ops.CHAIN_PERSIST_FWD = prev


# ---- an abandoned launch at the level of the step ------------------------------------------------------------------------------------
# After an abandoned launch every output of the chain is undefined except one NaN row per workgroup of the concat, and those rows do not
# reach the loss: every ReLU and hinge behind them is fmaxf, which drops a NaN operand -- the loss comes out as the finite m1 + m2 while
# the backward, the moving averages and Adam consume the rest.  The step therefore adds a verdict formed from the workspace's error word
# (ops.chain_persist_verdict) to the loss it returns.

def _tuple18(dev, seed, n=256):
    t = torch.from_numpy(O.synthetic_clouds(18, n, seed).reshape(1, 18, n, 3)).to(dev)
    return t[:, :1], t[:, 1:3], t[:, 3:17], t[:, 17:]


def _named_state(ts):
    names = ts.trainable_names()
    out = dict(ts.store.vars)
    out.update({k + "/Adam": ts.m[k] for k in names})
    out.update({k + "/Adam_1": ts.v[k] for k in names})
    return out


@pytest.mark.parametrize("form", ["eager", "graph"])
@pytest.mark.parametrize("precision", [None, "bf16"])
def test_abandoned_launch_reaches_the_step_loss(dev, precision, form):
    """A step whose persistent launch is abandoned (eager: a spin budget of one tick, a real abandonment; replayed: the sticky error word
    set, the budget being baked into the captured arguments) returns a NaN loss, not the finite MARGIN_1 + MARGIN_2; so does the next
    one; the status word says EPC_EHIP and the check raises and resets; and from the restored state the same step then gives the
    healthy run's loss and state bit for bit (the reset, the sequence advance, nothing stale in the graph's static buffers)."""
    L, ops, TR = H.pkg("lib"), H.pkg("ops"), H.pkg("training")
    lib = L.lib()
    graph = form == "graph"
    assert lib.epc_chain_persist_ok(18 * 256) == 1
    w0 = O.seeded_weights("epc-net", 4)
    params = dict(H.PARAMS, ARCH="epc-net", BATCH_NUM_QUERIES=1, BASE_LEARNING_RATE=1e-3, MARGIN_1=0.5, MARGIN_2=0.2)
    if precision is not None:
        params["TRAIN_PRECISION"] = precision
    T1, T2 = _tuple18(dev, 41), _tuple18(dev, 42)
    prev_ticks, prev_flag = ops.CHAIN_SPIN_TICKS, ops.CHAIN_PERSIST_FWD
    ops.CHAIN_PERSIST_FWD = True
    ws = ops.chain_workspace(dev)
    words = ws.view(torch.int32)
    try:
        # 1. the healthy run
        ts = TR.TrainStep(params, H.make_store("epc-net", w0, dev), outer=H.OUTER)
        ref_losses = [float(ts.step(*T, graph=graph)[0]) for T in (T1, T2)]
        ops.chain_persist_check()
        ref_state = {k: v.detach().clone() for k, v in _named_state(ts).items()}
        assert all(math.isfinite(x) for x in ref_losses) and ts.global_step == 2
        # 2., 3. a fresh identical store: T1 (in graph form the warm-up and the capture), snapshot
        ts = TR.TrainStep(params, H.make_store("epc-net", w0, dev), outer=H.OUTER)
        seq0 = _sequence_number(dev)
        assert float(ts.step(*T1, graph=graph)[0]) == ref_losses[0]
        assert _sequence_number(dev) > seq0                       # the step's forward is the persistent launch
        snap = {k: v.detach().clone() for k, v in _named_state(ts).items()}
        # 4. the next launch abandons
        if graph:
            words[ERR_WORD] = 1
        else:
            ops.CHAIN_SPIN_TICKS = 1
        # 5. the step on T2, and one more (the word is sticky)
        bad = [float(ts.step(*T2, graph=graph)[0]) for _ in range(2)]
        torch.cuda.synchronize()
        print("losses of the two steps behind an abandoned launch (%s, %s): %r; the healthy loss is %r, MARGIN_1 + MARGIN_2 = 0.7"
              % (precision or "bf16x6", form, bad, ref_losses[1]))
        assert lib.epc_chain_persist_status(ws.data_ptr(), L.current_stream()) == -3      # (or the rest passes vacuously)
        assert all(math.isnan(x) for x in bad), bad
        with pytest.raises(L.EpcNetError):
            ops.chain_persist_check()
        ops.CHAIN_SPIN_TICKS = prev_ticks
        torch.cuda.synchronize()
        assert int(words[ERR_WORD]) == 0
        # back to the state before the abandoned step: T2 is then the healthy run's second step, bit for bit
        state = _named_state(ts)
        with torch.no_grad():
            for k, v in snap.items():
                state[k].copy_(v)
        ts.global_step = 1
        ts.store.bump(ts.outer)
        assert float(ts.step(*T2, graph=graph)[0]) == ref_losses[1]
        ops.chain_persist_check()
        state = _named_state(ts)
        assert ts.global_step == 2 and sorted(state) == sorted(ref_state)
        differ = [k for k, v in ref_state.items() if not torch.equal(state[k], v)]
        assert not differ, differ[:10]
    finally:
        ops.CHAIN_SPIN_TICKS, ops.CHAIN_PERSIST_FWD = prev_ticks, prev_flag
        lib.epc_chain_persist_reset(ws.data_ptr(), L.current_stream())
        torch.cuda.synchronize()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_trainer_stops_on_an_abandoned_launch(dev, tmp_path, graph):
    """The training loop (the set-up of test_training_loop_with_mining_and_resume) stops at the FIRST step behind an abandoned launch:
    its non-finite-loss branch asks ops.chain_persist_check, which raises and resets, and the next epoch runs."""
    from test_gpu_kd_and_loop import N, _dataset
    L, ops, V, TR, TL = H.pkg("lib"), H.pkg("ops"), H.pkg("variables"), H.pkg("training"), H.pkg("train_loop")
    params = dict(H.PARAMS, ARCH="epc-net-l", BATCH_NUM_QUERIES=1, POSITIVES_PER_QUERY=2, NEGATIVES_PER_QUERY=6, NUM_POINTS=N,
                  BASE_LEARNING_RATE=1e-3, MAX_EPOCH=8)
    assert L.lib().epc_chain_persist_ok(10 * N) == 1
    queries, data = _dataset(40, N)
    st = V.reset_default_store(device=dev, seed=0)
    ts = TR.TrainStep(params, st)
    ts._ensure_built(N)
    st.randomize_statistics(0)
    tr = TL.Trainer(ts, queries, data, queries, data, save_path=str(tmp_path), logger=logging.getLogger("t"), graph=graph)
    np.random.seed(0)
    import random
    random.seed(0)
    prev_flag = ops.CHAIN_PERSIST_FWD
    ops.CHAIN_PERSIST_FWD = True
    ws = ops.chain_workspace(dev)
    try:
        seq0 = _sequence_number(dev)
        losses = tr.train_one_epoch(1, max_iters=2)
        assert len(losses) == 2 and all(np.isfinite(losses)) and _sequence_number(dev) > seq0      # (persistent launches)
        seen, step0 = len(tr.history), ts.global_step
        ws.view(torch.int32)[ERR_WORD] = 1
        with pytest.raises(L.EpcNetError):
            tr.train_one_epoch(2, max_iters=3)
        assert len(tr.history) - seen <= 1 and ts.global_step == step0 + 1      # it stopped at its first iteration
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32)[ERR_WORD]) == 0
        losses = tr.train_one_epoch(3, max_iters=3)
        assert len(losses) == 3 and all(np.isfinite(losses)), losses
    finally:
        ops.CHAIN_PERSIST_FWD = prev_flag
        L.lib().epc_chain_persist_reset(ws.data_ptr(), L.current_stream())
        torch.cuda.synchronize()
