"""epcnet_surfel_map_init / epcnet_surfel_map_add on the device (include/epcnet_growmap.h).  The reference of every bit comparison is
``surfel_ref.reference`` ON THE CONCATENATION of the calls -- the one-shot definition, never the code under test --; ``num_call`` is pinned
to the incremental restatement (tests/growmap_ref.py), whose count of voxels solved again is what shows that the work follows the rows
added.  Outputs, state and workspace are poisoned buffers of exactly the size asked for with slack behind them; everything is compared
on BIT PATTERNS."""
import ctypes
import functools
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import growmap_ref as G
import helpers as H
import localize_ref as Z
import map_ref as M
import register_ref as RR
import stage_ref as SG
import submap_ref as SR
import surfel_ref as S

pytestmark = pytest.mark.gpu

MP_TILE = 256            # MP_TILE of csrc/map_common.h: the rows of one insert / mark / number tile
MP_LEVEL = 256 * 256     # MP_TILE * MP_GROUP: the rows behind which the leaders' scan takes its second level
FLOATS = G.FLOATS
NAMES = ("map_points", "count", "centroid", "normal", "eigen", "support", "num_out")
SENTINEL = 0x12345678


def _up(a, dtype, dev):
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        return torch.zeros(12, dtype=torch.float64, device=dev).view(torch.from_numpy(a).dtype)      # a pointer that is never followed
    return torch.from_numpy(a).to(dev)


class _Dev:
    """The two entries themselves on poisoned buffers: a state of exactly epcnet_surfel_map_state_bytes, per call a workspace of exactly
    epcnet_surfel_map_add_workspace_bytes; after every call nothing was written behind any of them."""

    def __init__(self, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8):
        self.L = H.pkg("lib")
        self.dev = torch.device("cuda")
        self.max_voxels, self.ring = max_voxels, ring
        self.params = (ctypes.c_double * 8)(voxel, float(min_count), float(ring), float(min_support))
        self.origin = _up(origin, np.float64, self.dev)
        self.need = self.L.lib().epcnet_surfel_map_state_bytes(max_voxels)
        assert self.need > 0
        self.state = SG.Poisoned((self.need,), torch.uint8, self.dev)
        self.out = {name: SG.Poisoned((max_voxels, 3), torch.float32, self.dev) for name in FLOATS}
        self.out.update(count=SG.Poisoned((max_voxels,), torch.int32, self.dev), support=SG.Poisoned((max_voxels,), torch.int32, self.dev),
                        num_out=SG.Poisoned((4,), torch.int32, self.dev))
        self.init()

    def _arrays(self):
        return [self.out[name].t for name in NAMES]

    def init(self):
        self.L.run.epcnet_surfel_map_init(self.origin, self.params, self.max_voxels, self.state.t, self.need, *self._arrays())

    def add(self, points, offsets, poses, params=None, max_voxels=None):
        points = np.asarray(points, np.float32).reshape(-1, 3)
        rows, C = len(points), len(offsets) - 1
        need = self.L.lib().epcnet_surfel_map_add_workspace_bytes(rows, C, self.ring)
        assert need > 0
        ws, call = SG.Poisoned((need,), torch.uint8, self.dev), SG.Poisoned((4,), torch.int32, self.dev)
        self.L.run.epcnet_surfel_map_add(_up(points, np.float32, self.dev), _up(offsets, np.int32, self.dev), rows, C,
                                         _up(np.asarray(poses).reshape(-1, 12), np.float64, self.dev), self.params if params is None else params,
                                         self.max_voxels if max_voxels is None else max_voxels, self.state.t, self.need, *self._arrays(), call.t,
                                         ws.t, need)
        torch.cuda.synchronize()
        for p in list(self.out.values()) + [ws, call, self.state]:
            assert p.untouched()
        return call.t.cpu().tolist()

    def host(self):
        return {name: p.t.cpu().numpy() for name, p in self.out.items()}


def _check(got, want, what):
    assert got["num_out"].tolist() == want["num_out"].tolist(), (what, got["num_out"].tolist(), want["num_out"].tolist())
    for name in ("count", "support"):
        assert (got[name] == want[name]).all(), (what, name, int((got[name] != want[name]).sum()))
    for name in FLOATS:
        differ = (got[name].view(np.uint32) != want[name].view(np.uint32)).any(1).nonzero()[0]
        assert differ.size == 0, (what, name, "%d rows differ, the first is row %d" % (differ.size, int(differ[0])))


def _one_shot(kept, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8):
    return S.reference(*G.concatenation(kept), origin, voxel, max_voxels, min_count, ring, min_support)


def _sequence(calls, origin, voxel, max_voxels, what, every=True, **kw):
    """Every call through the device and through the restatement: num_call pinned exactly, and the outputs (after every call, or behind
    the last) against the one-shot reference on the concatenation of the valid calls -> ``(dev, reports, want)``."""
    dev, ref = _Dev(origin, voxel, max_voxels, **kw), G.Map(origin, voxel, max_voxels, **kw)
    _check(dev.host(), _one_shot([], origin, voxel, max_voxels, **kw), what + ": init")
    kept, reports, want = [], [], None
    for i, call in enumerate(calls):
        got = dev.add(*call)
        reports.append(ref.add(*call))
        assert got == reports[-1]["num_call"].tolist(), (what, "num_call of call %d" % i, got, reports[-1]["num_call"].tolist())
        if M.valid(call[1], len(call[0])):
            kept.append(call)
        if every or i == len(calls) - 1:
            want = _one_shot(kept, origin, voxel, max_voxels, **kw)
            _check(dev.host(), want, "%s: after call %d" % (what, i))
    return dev, reports, want


def _clouds(points, offsets, poses, first, last):
    """The clouds [first, last) of a packed scene as a call of their own."""
    offsets = np.asarray(offsets, np.int64)
    return (points[offsets[first]:offsets[last]], (offsets[first:last + 1] - offsets[first]).astype(np.int32),
            np.asarray(poses).reshape(-1, 12)[first:last])


NO_CLOUD = (np.zeros((0, 3), np.float32), np.array([0], np.int32), np.zeros((0, 12)))


def _no_rows(poses):
    return (np.zeros((0, 3), np.float32), np.array([0, 0, 0], np.int32), np.asarray(poses).reshape(-1, 12)[:2])


def _split(rows):
    """``rows`` rows over three clouds, the middle one empty, the last one a quarter."""
    return (rows - rows // 4, 0, rows // 4)


SIZES = [1, 63, 64, 65, MP_TILE - 1, MP_TILE, MP_TILE + 1, 3 * MP_TILE + 5]


@pytest.mark.parametrize("rows,ring", [(r, 1) for r in SIZES] + [(r, 0) for r in SIZES[:6]] + [(r, 2) for r in SIZES[:6]])
def test_row_counts_per_call(rows, ring):
    """Three calls of ``rows`` rows into one map, around the wave and the tile, with a call of no cloud and a call of no row between
    them; the scenes are 3 m wide so that their voxels have neighbours."""
    points, offsets, poses, origin = M.drive(3, _split(rows) * 3, extent=1.5)
    calls = [_clouds(points, offsets, poses, 3 * k, 3 * k + 3) for k in range(3)]
    calls = [calls[0], NO_CLOUD, calls[1], _no_rows(poses), calls[2]]
    dev, reports, want = _sequence(calls, origin, 0.5, 3 * rows, "3 x %d rows, ring %d" % (rows, ring), ring=ring, min_support=3)
    assert want["num_out"].tolist()[1:] == [3 * rows, 0, 0]
    assert reports[1]["num_call"].tolist() == [0, 0, 0, 0] and reports[3]["num_call"].tolist() == [0, 0, 0, 0]
    if rows >= 63:
        assert all(0 < r["num_call"][2] for r in reports[::2]) and reports[4]["num_call"][2] < want["V"]      # some solved again, never all
        assert ring == 0 or want["valid"].any()


def test_second_level_of_the_scan_in_the_second_call():
    """256 * 256 + 256 + 37 rows in the second call: its last 37 rows each open a voxel, so leaders sit behind the scan's first level
    (the group of the number is 1) as well as in front of it."""
    rng = np.random.default_rng(17)
    big = MP_LEVEL + MP_TILE + 37
    dense = rng.uniform(-1.5, 1.5, size=(big - 37, 3))
    lone = np.stack([100.0 + 1.5 * np.arange(37), np.zeros(37), np.zeros(37)], 1) + 0.25
    second = np.concatenate([dense, lone]).astype(np.float32)
    first, third = rng.uniform(-2.0, 0.0, size=(300, 3)).astype(np.float32), rng.uniform(99.0, 103.0, size=(300, 3)).astype(np.float32)
    poses = M.identity_poses(2, (3.0, -2.0, 1.0))
    calls = [(first, np.array([0, 100, 300], np.int32), poses), (second, np.array([0, 40000, big], np.int32), poses),
             (third, np.array([0, 300, 300], np.int32), poses)]
    dev, reports, want = _sequence(calls, np.array([3.0, -2.0, 1.0]), 0.5, 4096, "the scan's second level", every=False, min_support=3)
    lead = want["leader"]
    assert (lead >= 300 + MP_LEVEL + MP_TILE).sum() >= 37 and ((lead >= 300) & (lead < 300 + MP_LEVEL)).any()
    assert reports[1]["num_call"][0] > 100 and reports[2]["num_call"][2] < want["V"]


def _spread_scene():
    return M.drive(3, (70,) * 6, extent=1.5)


def test_untouched_rows_are_not_written():
    """Before the second add the output rows of the voxels the restatement calls clean are overwritten with a sentinel: behind the call
    they still hold it, and the dirty rows are the one-shot's."""
    points, offsets, poses, origin = _spread_scene()
    calls = [_clouds(points, offsets, poses, 0, 4), _clouds(points, offsets, poses, 4, 6)]
    for ring in (0, 1, 2):
        kw = dict(ring=ring, min_support=3)
        dev, ref = _Dev(origin, 0.5, 420, **kw), G.Map(origin, 0.5, 420, **kw)
        dev.add(*calls[0])
        ref.add(*calls[0])
        report = ref.add(*calls[1])
        clean, dirty = report["clean"], report["dirty"]
        assert len(clean) > 20 and len(dirty) > 10 and (len(dirty) > len(report["touched"])) == (ring > 0)
        at = torch.from_numpy(clean).to(dev.dev)
        for name in NAMES[:6]:
            dev.out[name].t.view(torch.int32)[at] = SENTINEL
        assert dev.add(*calls[1]) == report["num_call"].tolist()
        got, want = dev.host(), _one_shot(calls, origin, 0.5, 420, **kw)
        V = want["V"]
        for name in NAMES[:6]:
            bits, ref_bits = got[name].view(np.uint32), want[name].view(np.uint32)
            assert (bits[clean] == SENTINEL).all(), (ring, name, "a clean row was written")
            assert (bits[dirty] == ref_bits[dirty]).all(), (ring, name, "a dirty row")
            assert (bits[V:] == ref_bits[V:]).all(), (ring, name, "behind V")
        assert got["num_out"].tolist() == want["num_out"].tolist()


def _cells(cells, voxel=1.0, at=0.5):
    """One row inside each of the given integer cells (n, 3), at the fraction ``at`` of the cell."""
    return ((np.asarray(cells, np.float64) + at) * voxel).astype(np.float32)


@pytest.mark.parametrize("ring", [0, 1, 2])
def test_dense_block_and_a_second_call_on_one_face(ring):
    """5 x 5 x 5 cells around the origin with three rows each; the second call gives one more row to the 25 cells of the face x = 2 only:
    the cells with x >= 2 - ring are solved again, the others are not."""
    axis = np.arange(-2, 3)
    cells = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(31)
    block = np.concatenate([_cells(cells, 0.5, rng.uniform(0.02, 0.98, size=(125, 3))) for _ in range(3)])
    face = _cells(cells[cells[:, 0] == 2], 0.5, rng.uniform(0.02, 0.98, size=(25, 3)))
    calls = [(block, np.array([0, 200, 375], np.int32), M.identity_poses(2)), (face, np.array([0, 25], np.int32), M.identity_poses(1))]
    dev, reports, want = _sequence(calls, np.zeros(3), 0.5, 500, "block, ring %d" % ring, ring=ring, min_support=3)
    assert reports[0]["num_call"].tolist() == [125, 375, 125, 0] and reports[1]["num_call"].tolist() == [0, 25, 25 * (ring + 1), 0]
    g = want["vox"]["g"]
    inner, outer = int(np.nonzero((g == [2 - ring, 0, 0]).all(1))[0][0]), int(np.nonzero((g == [2, 2, 2]).all(1))[0][0])
    got = dev.host()
    assert got["count"][outer] == 4 and got["support"][inner] == 3 * (2 * ring + 1) ** 3 + (2 * ring + 1) ** 2
    assert want["valid"].all()


def test_neighbours_across_the_origin_and_past_the_range_edges_over_two_calls():
    """The scene of the one-shot entry's range test at voxel 1 -- voxels in the last cells of the range on x and in the first on y and x
    --, its rows dealt alternately to two calls: the mark step too must skip a cell out of range, never wrap it (a wrapped key names a cell
    that holds rows here)."""
    top = float(2 ** 20)
    rows = []
    for x in (top - 0.25, top - 0.5, top - 0.75, top - 1.5, top - 1.25):
        rows += [[x, 0.5, 0.5], [x, 0.25, -0.5]]
    for y in (-top, -top + 0.5, -top + 1.25):
        rows += [[0.5, y, 0.5], [-0.5, y, 0.25], [-0.25, y, -0.75]]
    rows += [[-top + 0.5, 1.5, 0.5], [-top + 0.25, 1.25, 0.5], [-top + 0.5, 0.5, 0.5], [top - 0.5, -1.5, 0.5], [top - 0.5, 1.5, 1.5]]
    rows += [[0.25, -0.25, 0.25], [-0.25, 0.25, -0.25], [-0.75, -0.5, 0.5], [0.5, 0.5, -0.5], [0.75, 0.25, 0.5]]     # around the origin
    points = np.array(rows, np.float32)
    assert (points.astype(np.float64) == np.array(rows)).all()
    pose = M.identity_poses(1)
    for ring in (1, 2):
        for order in ((points[0::2], points[1::2]), (points[1::2], points[0::2])):
            calls = [(p, np.array([0, len(p)], np.int32), pose) for p in order]
            dev, reports, want = _sequence(calls, np.zeros(3), 1.0, 64, "range edges, ring %d" % ring, ring=ring, min_support=3)
            g = want["vox"]["g"]
            assert g[:, 0].max() == 2 ** 20 - 1 and g[:, 1].min() == -2 ** 20 and g[:, 0].min() == -2 ** 20 and want["num_out"][3] == 0
            edge = int(np.nonzero((g == [2 ** 20 - 1, 0, 0]).all(1))[0][0])
            assert dev.host()["support"][edge] == (11 if ring == 1 else 12) and want["valid"].sum() > 8
            assert 0 < reports[1]["num_call"][2] <= want["V"]


def test_every_row_in_one_voxel_over_four_calls():
    """4 x 1024 rows in ONE voxel of 1 m: one slot, four epochs, the highest contention."""
    rng = np.random.default_rng(11)
    points = (rng.uniform(0.0, 1.0, size=(4096, 3)) * np.array([0.999, 0.999, 0.999])).astype(np.float32)
    poses = M.identity_poses(2, (7.0, -3.0, 2.0))
    calls = [(points[k * 1024:(k + 1) * 1024], np.array([0, 300, 1024], np.int32), poses) for k in range(4)]
    for max_voxels in (1, 8):
        dev, reports, want = _sequence(calls, np.zeros(3), 1.0, max_voxels, "one voxel, max_voxels %d" % max_voxels)
        assert [r["num_call"].tolist() for r in reports] == [[1, 1024, 1, 0]] + [[0, 1024, 1, 0]] * 3
        assert want["num_out"].tolist() == [1, 4096, 0, 0] and dev.host()["support"][0] == 4096


def test_every_row_its_own_voxel_and_overflow_by_one_in_the_last_call():
    """max_voxels == V is reached by the last call: the fullest table the contract allows.  With V - 1 the overflow falls in the last
    call -- everything NaN, -1 --, and a further call keeps it while the row counts go on."""
    rng = np.random.default_rng(12)
    cells = np.unique(rng.integers(-8, 8, size=(3000, 3)), axis=0)
    rng.shuffle(cells)
    V = len(cells)
    points = _cells(cells, 1.0, rng.uniform(0.05, 0.95, size=(V, 3)))
    pose = M.identity_poses(1)
    cuts = [0, V // 3, 2 * V // 3, V]
    calls = [(points[a:b], np.array([0, b - a], np.int32), pose) for a, b in zip(cuts[:-1], cuts[1:])]
    dev, reports, want = _sequence(calls, np.zeros(3), 1.0, V, "max_voxels == V", every=False, min_support=6)
    assert want["num_out"].tolist() == [V, V, 0, 0] and (want["count"] == 1).all() and 100 < want["valid"].sum() < V
    more = (points[:50], np.array([0, 50], np.int32), pose)
    dev, reports, want = _sequence(calls + [more], np.zeros(3), 1.0, V - 1, "max_voxels == V - 1", min_support=6)
    assert [r["num_call"][0] for r in reports] == [cuts[1], cuts[2] - cuts[1], -1, -1] and want["num_out"].tolist() == [-1, V + 50, 0, 0]
    got = dev.host()
    for name in FLOATS:
        assert (got[name].view(np.uint32) == M.NAN_WORD).all()
    assert not got["count"].any() and not got["support"].any()
    for max_voxels in (1, V // 2):
        _sequence(calls, np.zeros(3), 1.0, max_voxels, "overflow at max_voxels = %d" % max_voxels, min_support=6)


def test_stale_state_is_harmless():
    """A state that served one map serves another after init: numbers, epochs and sums of the first leave no trace.  And a voxel seen in
    call 1, left alone in call 2 and touched again in call 3: an epoch is compared for equality, not with 0."""
    points, offsets, poses, origin = _spread_scene()
    dev, _, _ = _sequence([_clouds(points, offsets, poses, 0, 3), _clouds(points, offsets, poses, 3, 6)], origin, 0.5, 420, "first life",
                          min_support=3)
    other = M.drive(9, (90, 60, 120), extent=2.0)
    calls = [_clouds(*other[:3], 0, 1), _clouds(*other[:3], 1, 3)]
    dev.origin.copy_(torch.from_numpy(other[3]))
    dev.init()
    torch.cuda.synchronize()
    ref = G.Map(other[3], 0.5, 420, min_support=3)
    _check(dev.host(), _one_shot([], other[3], 0.5, 420, min_support=3), "init over a used state")
    for i, call in enumerate(calls):
        assert dev.add(*call) == ref.add(*call)["num_call"].tolist()
        _check(dev.host(), _one_shot(calls[:i + 1], other[3], 0.5, 420, min_support=3), "second life, call %d" % i)
    # clouds 0 and 5 are 10 m apart: call 1 both, call 2 cloud 5's ground only, call 3 cloud 0's again
    again = SR.scan(777, 70, extent=1.5)
    calls = [_clouds(points, offsets, poses, 0, 6), _clouds(points, offsets, poses, 5, 6), (again, np.array([0, 70], np.int32), poses[:1])]
    dev, reports, want = _sequence(calls, origin, 0.5, 600, "touched, left alone, touched again", min_support=3)
    back = set(reports[2]["touched"]) & set(reports[0]["touched"]) & set(reports[1]["clean"])
    assert len(back) > 10 and len(reports[2]["clean"]) > 0


def test_a_refused_call_in_the_middle_adds_nothing():
    """Invalid offsets (decreasing, a negative first, a last behind the rows) and params whose bits differ from init's: the call reports
    -1, the seven outputs AND the state are unchanged bit for bit, and the next valid call matches the concatenation without it."""
    points, offsets, poses, origin = M.drive(4, (300, 0, 200, 150, 0, 250, 100), extent=2.0)
    first, middle, last = _clouds(points, offsets, poses, 0, 3), _clouds(points, offsets, poses, 3, 6), _clouds(points, offsets, poses, 6, 7)
    kw = dict(min_support=3)
    dev, ref = _Dev(origin, 0.5, 1000, **kw), G.Map(origin, 0.5, 1000, **kw)
    assert dev.add(*first) == ref.add(*first)["num_call"].tolist()
    before, state = dev.host(), dev.state.t.clone()
    refusals = []
    for at, value in ((1, 160), (0, -1), (3, 401)):
        bad = middle[1].copy()
        bad[at] = value
        assert not M.valid(bad, len(middle[0]))
        refusals.append(dict(offsets=bad))
    other = lambda **c: (ctypes.c_double * 8)(*[c.get(k, v) for k, v in (("voxel", 0.5), ("min_count", 1.0), ("ring", 1.0), ("min_support", 3.0))])
    refusals += [dict(params=other(voxel=0.5000000000000001)), dict(params=other(min_count=2.0)), dict(params=other(min_support=4.0)),
                 dict(max_voxels=999)]
    for change in refusals:
        got = dev.add(middle[0], change.get("offsets", middle[1]), middle[2], params=change.get("params"), max_voxels=change.get("max_voxels"))
        assert got == [-1, 0, 0, 0], (change, got)
        after = dev.host()
        for name in NAMES:
            assert (after[name].view(np.uint32) == before[name].view(np.uint32)).all(), (change, name)
        assert torch.equal(dev.state.t, state), (change, "the state")
    for i, call in enumerate((middle, last)):
        assert dev.add(*call) == ref.add(*call)["num_call"].tolist()
        _check(dev.host(), _one_shot([first, middle, last][:i + 2], origin, 0.5, 1000, **kw), "behind the refused calls, call %d" % i)


def test_nan_rows_rows_behind_the_offsets_and_a_nan_pose():
    points, offsets, poses, origin = M.drive(4, (300, 0, 0, 500, 0, 200), extent=2.0)
    first = _clouds(points, offsets, poses, 0, 1)
    rows = points[300:].copy()
    rows[7, 1], rows[299, 2], rows[300, 0], rows[499] = np.nan, np.inf, -np.inf, np.nan
    broken = poses[1:].copy()
    broken[4, 5] = np.nan                              # every row of the last cloud is absent
    second = (np.concatenate([SR.scan(999, 33), rows, SR.scan(998, 77)]), (offsets[1:] - 300 + 33).astype(np.int32), broken)
    third = _clouds(points, offsets, poses, 5, 6)
    dev, reports, want = _sequence([first, second, third], origin, 0.5, 1000, "non-finite rows, a NaN pose, rows of no cloud", min_support=3)
    assert [r["num_call"][1] for r in reports] == [300, 496, 200] and want["num_out"].tolist()[1:] == [996, 204, 0]
    dev, reports, want = _sequence([first, second], np.array([0.0, np.nan, 0.0]), 0.5, 1000, "a NaN origin", min_support=3)
    assert want["num_out"].tolist() == [0, 0, 1000, 0]
    dev, reports, want = _sequence([first, second], np.zeros(3), 0.5, 1000, "origin 0: out of range", min_support=3)
    assert want["num_out"].tolist() == [0, 0, 204, 796]


def _planar_scene():
    """Rows exactly on the plane x + 2 y + 2 z = 0 and on the lattice of voxel / 256 (voxel 1): a (2, -1, 0) + b (0, 1, -1), in 1 / 256."""
    rng = np.random.default_rng(41)
    ab = rng.integers(-380, 381, size=(3000, 2))
    p = (ab[:, :1] * np.array([2, -1, 0]) + ab[:, 1:] * np.array([0, 1, -1])) / 256.0
    return p.astype(np.float32), np.array([0, 1000, 3000], np.int32), M.identity_poses(2, (4.0, -2.0, 8.0)), np.array([4.0, -2.0, 8.0])


def _contracted(N, S1, S2):
    """C with fl(fl(S2 / N) - fl(mu_a mu_b)) contracted to ONE fused operation, fma(-mu_a, mu_b, fl(S2 / N)), rounded once."""
    mu, C = S.covariance(N, S1, S2)
    out = C.copy()
    for j in range(len(N)):
        for k, (a, b) in enumerate(S._AB):
            out[j, k] = float(F(float(np.float64(S2[j, k]) / np.float64(N[j]))) - F(float(mu[j, a])) * F(float(mu[j, b])))
    return mu, out


def test_planar_lattice_scene_over_two_calls():
    """The scene on which a contracted multiply-add in C_ab changes float32 outputs (re-counted here), one cloud per call: the shared
    solve keeps contract(off) in this file's kernels too."""
    points, offsets, poses, origin = _planar_scene()
    calls = [_clouds(points, offsets, poses, 0, 1), _clouds(points, offsets, poses, 1, 2)]
    dev, reports, want = _sequence(calls, origin, 1.0, 3000, "planar", min_support=6)
    ok, V = want["valid"], want["V"]
    N, S1, S2 = (v[ok] for v in want["pooled"])
    lam2, n2 = S.order_and_normal(*S.jacobi(_contracted(N, S1, S2)[1]))
    fused = S.finish(want["vox"]["g"][ok], _contracted(N, S1, S2)[0], lam2, n2, 1.0)
    mine = [want[name][:V][ok] for name in ("centroid", "normal", "eigen")]
    changed = int(np.any([(a.view(np.uint32) != b.view(np.uint32)).any(1) for a, b in zip(mine, fused)], 0).sum())
    assert ok.sum() > 30 and changed > ok.sum() // 3
    got = dev.host()
    n = got["normal"][:V][ok].astype(np.float64)
    assert (np.abs(n - np.array([1.0, 2.0, 2.0]) / 3.0) < 1e-6).all() and (got["eigen"][:V][ok][:, 0] < 1e-12).all()
    assert reports[1]["num_call"][2] >= reports[1]["num_call"][0] >= 0 and reports[1]["num_call"][2] > 0


@pytest.mark.parametrize("voxel", [0.2, 0.5])
def test_utm_sized_poses_with_general_rotations_over_three_calls(voxel):
    points, offsets, poses, origin = M.drive(1, (2000,) * 4)
    points = points.copy()
    points[::97, 0] = np.nan
    calls = [_clouds(points, offsets, poses, 0, 2), _clouds(points, offsets, poses, 2, 3), _clouds(points, offsets, poses, 3, 4)]
    dev, reports, want = _sequence(calls, origin, voxel, 8000, "UTM, voxel %g" % voxel, every=False, min_support=3)
    assert want["num_out"].tolist()[1:] == [7917, 83, 0] and np.abs(poses.reshape(-1, 3, 4)[:, 0, 3]).min() > 5e6
    assert want["valid"].sum() > (2000 if voxel == 0.5 else 50) and all(0 < r["num_call"][2] <= want["V"] for r in reports)


def _dev(points, offsets, poses, origin=None):
    dev = torch.device("cuda")
    out = (torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev), torch.from_numpy(np.asarray(offsets, np.int32)).to(dev),
           torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev))
    return out if origin is None else out + (torch.from_numpy(np.ascontiguousarray(origin, np.float64)).to(dev),)


def _host(m):
    return {name: getattr(m, name).cpu().numpy() for name in NAMES}


def test_one_graph_replayed_three_times_on_other_inputs():
    """ONE captured add, replayed on three different inputs of the same shape against one state (graph nodes have misbehaved from the
    second replay on, hence three): the one-shot on the concatenation; from reset() the same bits again."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets, poses, origin = M.drive(21, (600, 500, 400) * 3, extent=3.0)
    calls = [_clouds(points, offsets, poses, 3 * k, 3 * k + 3) for k in range(3)]
    refs = [S.reference(*G.concatenation(calls[:k + 1]), origin, 0.5, 4500, 1, 1, 4) for k in range(3)]
    assert refs[0]["V"] < refs[1]["V"] < refs[2]["V"] and refs[2]["valid"].sum() > 50
    kw = dict(max_voxels=4500, voxel=0.5, origin=_dev(*calls[0], origin)[3], min_count=1, ring=1, min_support=4)
    pts, off, pos = _dev(*calls[0])
    ws = torch.empty(L.lib().epcnet_surfel_map_add_workspace_bytes(1500, 3, 1), dtype=torch.uint8, device=dev)
    ops.SurfelMap(**kw).add(pts, off, pos, workspace=ws)                      # (warm-up, on a map of its own)
    m = ops.SurfelMap(**kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        num_call = m.add(pts, off, pos, workspace=ws)
    ref = G.Map(origin, 0.5, 4500, 1, 1, 4)
    runs = []
    for life in range(2):
        for k, call in enumerate(calls):
            for dst, src in zip((pts, off, pos), _dev(*call)):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            _check(_host(m), refs[k], "life %d, replay %d" % (life, k))
            assert num_call.tolist() == ref.add(*call)["num_call"].tolist()
        runs.append(_host(m))
        m.reset()
        ref.reset()
    for name in NAMES:
        assert (runs[0][name].view(np.uint32) == runs[1][name].view(np.uint32)).all(), name


def test_wrapper_its_defaults_and_refusals():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets, poses, origin = M.drive(8, (1200, 800), extent=2.0)
    a, b = _dev(*_clouds(points, offsets, poses, 0, 1)), _dev(*_clouds(points, offsets, poses, 1, 2))
    org = torch.from_numpy(origin).to(dev)
    m = ops.SurfelMap(2000, origin=org)                                       # voxel 0.2, min_count 1, ring 1, min_support 8
    assert m.origin is org and [tuple(getattr(m, n).shape) for n in NAMES] == [(2000, 3), (2000,), (2000, 3), (2000, 3), (2000, 3), (2000,), (4,)]
    assert m.num_out.tolist() == [0, 0, 0, 0] and not m.count.any() and torch.isnan(m.normal).all()
    tensors = [getattr(m, n) for n in NAMES]
    first = m.add(*a)
    assert first.is_cuda and first.dtype == torch.int32 and tuple(first.shape) == (4,)
    _check(_host(m), S.reference(points[:1200], [0, 1200], poses[:1], origin, 0.2, 2000), "one call")
    m.add(b[0], b[1], b[2].reshape(1, 3, 4))
    want = S.reference(points, offsets, poses, origin, 0.2, 2000)
    _check(_host(m), want, "two calls")
    assert np.isfinite(want["normal"]).all(1).sum() > 30 and all(getattr(m, n) is t for n, t in zip(NAMES, tensors))
    fused = ops.fuse_surfels(*_dev(points, offsets, poses), origin=org, max_voxels=2000)
    for name, theirs in zip(NAMES, fused[:7]):
        assert torch.equal(getattr(m, name).view(torch.int32), theirs.view(torch.int32)), name
    m.reset()
    assert m.num_out.tolist() == [0, 0, 0, 0] and torch.isnan(m.map_points).all() and all(getattr(m, n) is t for n, t in zip(NAMES, tensors))
    m.add(*b)
    _check(_host(m), S.reference(points[1200:], [0, 800], poses[1:], origin, 0.2, 2000), "after reset()")
    own = ops.SurfelMap(2000, voxel=0.5, min_count=2, ring=2, min_support=20)                  # origin=None: the first add's first translation
    assert own.origin is None
    need = L.lib().epcnet_surfel_map_add_workspace_bytes(1200, 1, 2)
    own.add(*a, workspace=torch.full((need,), 0xAB, dtype=torch.uint8, device=dev))
    assert own.origin.is_cuda and own.origin.dtype == torch.float64 and own.origin.tolist() == poses[0, 3::4].tolist()
    assert own.origin.data_ptr() != a[2].data_ptr() + 24
    kept = own.origin
    own.add(*b)
    assert own.origin is kept
    ref = S.reference(points, offsets, poses, origin, 0.5, 2000, 2, 2, 20)
    assert ref["num_out"][0] > 0
    _check(_host(own), ref, "origin=None, a caller's workspace")
    with pytest.raises(L.EpcNetError) as e:
        own.add(*a, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.status == L.EPC_ENOMEM
    with pytest.raises(L.EpcNetError) as e:
        own.add(a[0], a[1], a[2].float())
    assert "float64" in str(e.value) and "never converted" in str(e.value)
    for change in (dict(points=a[0].cpu()), dict(offsets=a[1].cpu()), dict(offsets=a[1].long()), dict(poses=a[2].cpu()), dict(poses=b[2][:0]),
                   dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device=dev)), dict(workspace=torch.empty(1 << 20, dtype=torch.uint8))):
        with pytest.raises(L.EpcNetError):
            own.add(**dict(dict(points=a[0], offsets=a[1], poses=a[2]), **change))
    _check(_host(own), ref, "refusals change nothing")
    for bad in (dict(max_voxels=0), dict(max_voxels=2 ** 28 + 1), dict(ring=-1), dict(ring=3), dict(ring=0.5), dict(min_support=2),
                dict(min_support=8.5), dict(origin=org.cpu()), dict(origin=org.float()), dict(voxel=0.0, origin=org),
                dict(min_count=0, origin=org)):
        with pytest.raises(L.EpcNetError):
            ops.SurfelMap(**dict(dict(max_voxels=100), **bad))


def test_the_loop_once():
    """A map from three submaps, index_surfels, localize_scans of one 1024-row cloud from a perturbed seed, add at the returned pose:
    bit-equal to fuse_surfels over the four clouds with that pose appended (read back only for the comparison)."""
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    patches = [p.astype(np.float32) for p in Z.plane_patches(5, *Z.THREE_PLANES, 3000)]
    sub_points, sub_offsets = SR.pack(patches)
    fixed = M.identity_poses(3)
    truth = RR.pose_of(3.0, -2.0, 1.5, (0.05, -0.04, 0.03))
    cloud = Z.plane_scan(77, *Z.THREE_PLANES, 1024, truth)
    origin = torch.zeros(3, dtype=torch.float64, device=dev)
    m = ops.SurfelMap(max_voxels=16384, voxel=0.2, origin=origin)
    pts, off, pos = _dev(sub_points, sub_offsets, fixed)
    m.add(pts, off, pos)
    index, num = ops.index_surfels(m.map_points, m.centroid, m.normal, 0.2)
    seeds = torch.from_numpy(np.asarray(RR.IDENTITY, np.float64).reshape(1, 1, 12)).to(dev)
    scan = torch.from_numpy(cloud).to(dev)
    pose, fit, hessian, info, status = ops.localize_scans(scan[None], index, m.centroid, m.normal, seeds)
    scan_offsets = torch.tensor([0, 1024], dtype=torch.int32, device=dev)
    num_call = m.add(scan, scan_offsets, pose)
    assert status.tolist() == [0] and torch.isfinite(pose).all() and int(num[0]) > 500
    assert float((pose.cpu().reshape(3, 4)[:, 3] - torch.from_numpy(np.asarray(truth).reshape(3, 4)[:, 3])).abs().max()) < 0.05
    fused = ops.fuse_surfels(torch.cat([pts, scan]), torch.cat([off, off[-1:] + 1024]), torch.cat([pos, pose]), voxel=0.2, origin=origin,
                             max_voxels=16384)
    for name, theirs in zip(NAMES, fused[:7]):
        assert torch.equal(getattr(m, name).view(torch.int32), theirs.view(torch.int32)), name
    assert 0 < int(num_call[2]) <= int(m.num_out[0]) and int(num_call[1]) == 1024
