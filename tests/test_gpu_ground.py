"""epcnet_ground_remove on the device against its numpy restatement (tests/ground_ref.py): every comparison is on bit patterns, there is no
tolerance anywhere -- the definition is float32 with one rounding per operation and integer counts.  Ragged batches around the
scorer's tile, scans that share a tile, position independence, the degenerate scans, bad offsets, in place, the engine's raw-scan entry
with the removal in front, a captured graph replayed on another batch, the refusals."""
import functools

import numpy as np
import pytest
import torch

import downsample_ref as D
import ground_ref as G
import helpers as H
import stage_ref as S
from helpers import O

pytestmark = pytest.mark.gpu

T = 1024        # GR_TILE of csrc/ground.hip: the rows of one scorer tile


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _tiny(M):
    return D.scene(7, 40 + M)[:M]


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "tiles":      # a 5-row scan in front (every later scan starts at an odd row), five scans inside one tile, the tile's edges
        return tuple([D.scene(5, 99)] + [_tiny(M) for M in (0, 1, 2, 3, 7)] + [D.scene(M, M) for M in (T - 1, T, T + 1, 3 * T + 5)]
                     + [D.scene(20000, 20000)])
    if name == "short":
        return (D.scene(5, 99), _tiny(3), D.scene(T + 1, T + 1), G.family(1)[:9000])
    if name == "alone":
        return (G.family(4)[:70000],)
    if name == "three":
        return (G.wall_only(5000, 1), G.cube(5000, 2), G.family(2)[:30001])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name, hypotheses=256, draws=8):
    return G.reference_batch(_batch(name), hypotheses=hypotheses, draws=draws)


def _run(scans, **kw):
    ops = H.pkg("ops")
    points, offsets = ops.pack_scans(list(scans))
    got = ops.remove_ground(points, offsets, **kw)
    assert all(t.is_cuda for t in got) and got[0].dtype == got[2].dtype == torch.float32 and got[1].dtype == got[3].dtype == torch.int32
    return tuple(t.cpu() for t in got)


def _check(got, want, what):
    out, status, plane, info = got
    ro, rs, rp, ri = (torch.from_numpy(a) for a in want)
    assert torch.equal(info, ri), (what, info.tolist(), ri.tolist())         # where a mismatch began: finite rows, valid, best h, score
    assert torch.equal(status, rs), (what, status.tolist(), rs.tolist())
    assert _same(plane, rp), (what, plane.tolist(), rp.tolist())
    assert out.shape == ro.shape
    differ = (_bits(out) != _bits(ro)).any(1).nonzero()
    assert differ.numel() == 0, (what, "%d rows differ, the first is row %d" % (differ.numel(), int(differ[0])))


def test_tile_edges_and_scans_that_share_a_tile():
    want = _reference("tiles")
    assert want[1].tolist()[1:5] == [8] * 4 and want[1].tolist()[6:] == [0] * 5 and want[3][1].tolist() == [0, 0, -1, 0]
    assert int(np.isnan(want[0]).all(1).sum()) > 10000
    _check(_run(_batch("tiles")), want, "tiles")


@pytest.mark.parametrize("hypotheses,draws", [(64, 1), (1024, 16)])
def test_fewest_and_most_hypotheses_and_draws(hypotheses, draws):
    want = _reference("short", hypotheses, draws)
    assert want[1].tolist()[2:] == [0, 0]
    _check(_run(_batch("short"), hypotheses=hypotheses, draws=draws), want, "H=%d K=%d" % (hypotheses, draws))


def test_one_large_scan_alone():
    want = _reference("alone")
    assert want[1].tolist() == [0]
    _check(_run(_batch("alone")), want, "70 000 rows, B = 1")


def test_degenerate_scans_beside_a_good_one_and_position_independence():
    scans, want = _batch("three"), _reference("three")
    assert want[1].tolist() == [8, 8, 0] and want[3][0].tolist() == [5000, 0, -1, 0]
    got = _run(scans)
    _check(got, want, "wall, cube, good")
    packed = torch.from_numpy(np.concatenate(scans))
    assert _same(got[0][:10000], packed[:10000])                             # the two failed scans: untouched bits
    ends = np.cumsum([0] + [len(s) for s in scans])
    for order in ((2, 0, 1), (1, 2, 0)):
        out, status, plane, info = _run([scans[i] for i in order])
        at = 0
        for i in order:                                                      # every scan: the bits it had in the first order
            m = len(scans[i])
            assert _same(out[at:at + m], got[0][ends[i]:ends[i + 1]]), (order, i)
            at += m
        assert _same(status, got[1][list(order)]) and _same(plane, got[2][list(order)]) and _same(info, got[3][list(order)])


def test_in_place_and_twice():
    ops = H.pkg("ops")
    points, offsets = ops.pack_scans(list(_batch("short")))
    before = points.clone()
    a = ops.remove_ground(points, offsets)
    assert _same(points, before) and a[0].data_ptr() != points.data_ptr()     # out of place: the input is left alone
    b = ops.remove_ground(points, offsets)
    assert all(_same(x, y) for x, y in zip(a, b))
    c = ops.remove_ground(points, offsets, out=points)
    assert c[0].data_ptr() == points.data_ptr() and all(_same(x, y) for x, y in zip(a, c))
    _check(tuple(t.cpu() for t in c), _reference("short"), "in place")
    # another seed is another draw: the words say so, and the restatement follows
    d = tuple(t.cpu() for t in ops.remove_ground(before, offsets, seed=-(1 << 63) + 12345))
    assert not _same(d[3], a[3].cpu())
    _check(d, G.reference_batch(_batch("short"), seed=-(1 << 63) + 12345), "seed")


def test_bad_offsets_fail_every_scan_and_copy_the_rows():
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    a, b = D.scene(2000, 1), D.scene(3000, 2)
    rows = np.concatenate([a, b])
    points = torch.from_numpy(rows).to(dev)
    for offs in ([0, 2000, 1500, 5000], [-1, 2000, 2000, 5000], [0, 2000, 2000, 5001]):
        offsets = torch.tensor(offs, dtype=torch.int32, device=dev)
        out, status, plane, info = ops.remove_ground(points, offsets)
        assert status.tolist() == [8, 8, 8] and info.tolist() == [[0, 0, 0, 0]] * 3 and bool(torch.isnan(plane).all()), offs
        assert _same(out, points), offs
    # valid offsets that leave rows outside every scan: those rows are copied, the scans are the restatement's
    offsets = torch.tensor([7, 2000, 2000, 4990], dtype=torch.int32, device=dev)
    out, status, plane, info = (t.cpu() for t in ops.remove_ground(points, offsets))
    want = G.reference_batch([rows[7:2000], rows[2000:2000], rows[2000:4990]])
    assert status.tolist() == [0, 8, 0]
    _check((out[7:4990], status, plane, info), want, "rows outside the scans")
    assert _same(out[:7], points[:7].cpu()) and _same(out[4990:], points[4990:].cpu())


def test_a_scan_above_the_row_limit_fails_alone():
    big = np.tile(D.scene(4099, 5), (256, 1))[:(1 << 20) + 1]
    scans = (D.scene(3000, 3), big, D.scene(2000, 4))
    want = G.reference_batch(scans)
    assert want[1].tolist() == [0, 8, 0] and want[3][1].tolist() == [0, 0, 0, 0]
    _check(_run(scans), want, "2^20 + 1 rows between two good scans")


def test_max_z_picks_the_plane_below_the_sensor():
    roofed = G.roofed(0)
    for max_z, height in ((float("inf"), 3.0), (0.0, -1.8)):
        want = G.reference_batch([roofed], max_z=max_z)
        assert want[1].tolist() == [0] and abs(want[2][0][3] / want[2][0][2] - height) < 0.1
        _check(_run([roofed], max_z=max_z), want, "max_z=%r" % max_z)


def test_outputs_end_where_they_should():
    """The entry itself on output buffers filled with 0xFF bytes that have slack behind them, info NULL, the workspace of exactly the
    size asked for."""
    L, ops = H.pkg("lib"), H.pkg("ops")
    dev = torch.device("cuda")
    scans = _batch("short")
    points, offsets = ops.pack_scans(list(scans))
    rows, B = int(points.shape[0]), len(scans)
    want = _reference("short")
    need = L.lib().epcnet_ground_workspace_bytes(B, 256, rows)
    for with_info in (True, False):
        out, plane = S.Poisoned((rows, 3), torch.float32, dev), S.Poisoned((B, 4), torch.float32, dev)
        info, status = S.Poisoned((B, 4), torch.int32, dev), S.Poisoned((B,), torch.int32, dev)
        ws = S.Poisoned((need,), torch.uint8, dev)
        L.run.epcnet_ground_remove(points, offsets, rows, B, 256, 8, 0.2, float(G.cos2_of(15.0)), float("inf"), 0.05, 0, out.t, plane.t,
                                   info.t if with_info else None, status.t, ws.t, need)
        torch.cuda.synchronize()
        assert out.untouched() and plane.untouched() and info.untouched() and status.untouched() and ws.untouched()
        if with_info:
            _check((out.t.cpu(), status.t.cpu(), plane.t.cpu(), info.t.cpu()), want, "poisoned outputs")
        else:
            assert S.holds_poison(info.t) and _same(out.t.cpu(), torch.from_numpy(want[0]))


@functools.lru_cache(maxsize=None)
def _engine_scans():
    return (G.family(11)[:6000], D.scene(60, 22), G.wall_only(3000, 23), G.family(12)[:4777])


def test_engine_forward_scans_with_ground_and_its_graph():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    arch = "epc-net-l"
    eng, _ = H.make_engine(arch, O.seeded_weights(arch, 0), dev, in_flight=1)
    points, offsets = ops.pack_scans(list(_engine_scans()))
    kept, st_ground, _, _ = ops.remove_ground(points, offsets)
    xyz, st_ds, _ = ops.grid_downsample(kept, offsets, 256)
    want = eng.forward(xyz).clone()
    desc, status = eng.forward_scans(points, offsets, num_points=256, ground=True)
    assert _same(desc, want) and _same(status, st_ds | st_ground)
    # the 60-row scene loses its ground and then has no grid; the wall has no ground and goes on as it came
    assert status.tolist() == [0, L.EPC_STATUS_NO_GRID, L.EPC_STATUS_NO_GROUND, 0]
    assert bool(torch.isnan(desc[1]).all()) and bool(torch.isfinite(desc[[0, 2, 3]]).all())
    as_dict, st_dict = eng.forward_scans(points, offsets, num_points=256, ground=dict(hypotheses=128, draws=4, seed=3))
    k2 = ops.remove_ground(points, offsets, hypotheses=128, draws=4, seed=3)[0]
    assert _same(as_dict, eng.forward(ops.grid_downsample(k2, offsets, 256)[0])) and st_dict.tolist() == status.tolist()
    # ground=None is the call without the argument
    plain = eng.forward(ops.grid_downsample(points, offsets, 256)[0]).clone()
    d0, s0 = eng.forward_scans(points, offsets, num_points=256)
    d0 = d0.clone()
    d1, s1 = eng.forward_scans(points, offsets, num_points=256, ground=None)
    assert _same(d0, plain) and _same(d1, plain) and _same(s0, s1) and s0.tolist() == [0, L.EPC_STATUS_NO_GRID, 0, 0]
    assert not _same(plain[0], want[0])                                      # the ground was part of the descriptor

    # captured on one stream, replayed ONCE after the buffers were overwritten with another batch of the same rows and B
    other = [G.family(13)[:5000], G.family(14)[:5837], G.wall_only(3000, 15), np.zeros((0, 3), np.float32)]
    assert sum(len(s) for s in other) == sum(len(s) for s in _engine_scans())
    p2, o2 = ops.pack_scans(other)
    eager, eager_status = eng.forward_scans(p2, o2, num_points=256, ground=True)
    eager, eager_status = eager.clone(), eager_status.clone()
    out = torch.empty((4, 256), dtype=torch.float32, device=dev)
    eng.forward_scans(points, offsets, num_points=256, out=out, ground=True)  # (warm-up: weights packed, workspace allocated before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, st_graph = eng.forward_scans(points, offsets, num_points=256, out=out, ground=True)
    points.copy_(p2)
    offsets.copy_(o2)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, eager) and _same(st_graph, eager_status)
    assert eager_status.tolist() == [0, 0, L.EPC_STATUS_NO_GROUND, L.EPC_STATUS_NO_GROUND | L.EPC_STATUS_NO_GRID]


def test_refusals_write_nothing():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets = ops.pack_scans([D.scene(2000, 1)])
    good = dict(hypotheses=256, draws=8, threshold=0.2, max_tilt_deg=15.0, min_share=0.05, max_z=float("inf"))
    for bad in (dict(hypotheses=100), dict(hypotheses=32), dict(hypotheses=1088), dict(draws=0), dict(draws=17), dict(threshold=0.0),
                dict(threshold=float("nan")), dict(max_tilt_deg=90.0), dict(max_tilt_deg=-1.0), dict(min_share=1.5), dict(max_z=float("nan"))):
        out = torch.full((2000, 3), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(L.EpcNetError):
            ops.remove_ground(points, offsets, out=out, **dict(good, **bad))
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), bad
    with pytest.raises(L.EpcNetError):
        ops.remove_ground(points.cpu(), offsets)
    with pytest.raises(L.EpcNetError):
        ops.remove_ground(points, offsets.long())
    with pytest.raises(L.EpcNetError):
        ops.remove_ground(points, offsets, out=torch.empty((1999, 3), dtype=torch.float32, device=dev))
    # the entry itself: a refused call and a short workspace leave every output as it was
    need = L.lib().epcnet_ground_workspace_bytes(1, 256, 2000)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    for hyp, size, code in ((100, need, L.EPC_EINVAL), (256, need - 1, L.EPC_ENOMEM)):
        out = torch.full((2000, 3), 7.0, dtype=torch.float32, device=dev)
        plane = torch.full((1, 4), 7.0, dtype=torch.float32, device=dev)
        info, status = torch.full((1, 4), -7, dtype=torch.int32, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
        with pytest.raises(L.EpcNetError) as e:
            L.run.epcnet_ground_remove(points, offsets, 2000, 1, hyp, 8, 0.2, 0.9, float("inf"), 0.05, 0, out, plane, info, status, ws, size)
        torch.cuda.synchronize()
        assert e.value.status == code
        assert bool((out == 7.0).all()) and bool((plane == 7.0).all()) and bool((info == -7).all()) and status.item() == -7
    # no scan at all: the rows are copied; no row at all: the words are written
    empty_offsets = torch.zeros(1, dtype=torch.int32, device=dev)
    out, status, plane, info = ops.remove_ground(points, empty_offsets)
    assert _same(out, points) and status.numel() == 0 and tuple(plane.shape) == (0, 4)
    out, status, plane, info = ops.remove_ground(points[:0], torch.zeros(3, dtype=torch.int32, device=dev))
    assert tuple(out.shape) == (0, 3) and status.tolist() == [8, 8] and info.tolist() == [[0, 0, -1, 0]] * 2
