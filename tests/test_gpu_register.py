"""epcnet_pair_register on the device against tests/register_ref.py, the numpy restatement of include/epcnet_pairs.h -- never the entry under
test.  Every output goes into a poisoned buffer with guard bytes IN FRONT of it and behind it, the workspace is exactly the size asked for,
``pose`` and ``fit`` are compared on BIT PATTERNS, ``info`` and ``status`` exactly: ICP's correspondences are discrete, so there is no
tolerance anywhere.  The grid of n x P x H x iterations around the wave and the chunk of 256 rows, the cloud that fills the LDS, ties on a
lattice, absent rows, the flags, the refusals, two runs, one captured graph replayed on other data, the Python entries and a small
out-and-back drive through the engine."""
import numpy as np
import pytest
import torch

import helpers as H
import register_ref as R
import submap_ref as SR
from helpers import Guarded, O

pytestmark = pytest.mark.gpu


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to("cuda")


def _raw(clouds, pairs, seeds, max_dist, iterations, min_pairs):
    """The entry itself on guarded, poisoned outputs and a guarded workspace of exactly the size asked for -> (pose, fit, info, status)."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    C, n, P = clouds.shape[0], clouds.shape[1], len(pairs)
    Hs = 1 if seeds is None else seeds.shape[1]
    need = L.lib().epcnet_pair_register_workspace_bytes(P, Hs, n)
    assert need > 0 and need % 16 == 0
    pose, fit = Guarded((P, 12), torch.float64, dev), Guarded((P, 2), torch.float64, dev)
    info, status = Guarded((P, 4), torch.int32, dev), Guarded((P,), torch.int32, dev)
    ws = Guarded((need,), torch.uint8, dev)
    L.run.epcnet_pair_register(_up(clouds, np.float32), C, n, _up(pairs, np.int32), P, None if seeds is None else _up(seeds, np.float64), Hs,
                               float(max_dist), iterations, min_pairs, pose.t, fit.t, info.t, status.t, ws.t, need)
    torch.cuda.synchronize()
    for g in (pose, fit, info, status, ws):
        assert g.intact()
    return pose.t.cpu().numpy(), fit.t.cpu().numpy(), info.t.cpu().numpy(), status.t.cpu().numpy()


def _equal(got, want, what):
    gp, gf, gi, gs = got
    wp, wf, wi, ws = want
    assert gs.tolist() == ws.tolist(), (what, "status")
    assert gi.tolist() == wi.tolist(), (what, "info")
    for name, g, w in (("pose", gp, wp), ("fit", gf, wf)):
        bad = np.nonzero((np.ascontiguousarray(g).view(np.int64) != np.ascontiguousarray(w).view(np.int64)).any(1))[0]
        assert bad.size == 0, (what, name, "%d pairs differ, the first is %d: %s / %s" % (bad.size, bad[0], g[bad[0]].tolist(), w[bad[0]].tolist()))


def _both(clouds, pairs, seeds, max_dist, iterations, min_pairs, what, memo=None):
    want = R.register_reference(clouds, pairs, seeds, max_dist, iterations, min_pairs, memo=memo)
    got = _raw(clouds, np.asarray(pairs, np.int32).reshape(-1, 2), seeds, max_dist, iterations, min_pairs)
    _equal(got, want, what)
    return got


def _moved_clouds(seed, n, count=6, noise=0.02):
    """`count` views of one structured scene of n rows: each under its own small motion, with its own noise and row order."""
    rng = np.random.default_rng([seed, n, 5])
    scene = R.structured_scene(seed, n)
    out = []
    for c in range(count):
        m = R.pose_of(rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.8, 0.8, size=3))
        out.append((R.apply_pose(m, scene) + noise * rng.normal(size=scene.shape))[rng.permutation(n)])
    return np.stack(out).astype(np.float32)


def _seeds_for(seed, P, Hs):
    rng = np.random.default_rng([seed, P, Hs, 9])
    return np.stack([[R.pose_of(*rng.uniform(-6, 6, size=3), rng.uniform(-0.6, 0.6, size=3)) for _ in range(Hs)] for _ in range(P)])


@pytest.mark.parametrize("n", [32, 64, 96, 224, 256, 288, 1024])
def test_grid_of_sizes(n):
    """P in {1, 3, 17} x H in {1, 4} x iterations in {0, 1, 5}.  The pairs of a smaller P are a prefix of the larger's and H = 1 takes the
    first of the four seeds, so the restatement's passes are shared through its memo; P = 3 with H = 1 runs without seeds (the identity)."""
    clouds = _moved_clouds(n, n)
    rng = np.random.default_rng([n, 17])
    pairs = np.stack([rng.integers(0, 6, size=17), rng.integers(0, 6, size=17)], 1).astype(np.int32)
    seeds = _seeds_for(n, 17, 4)
    memo = {}
    ran = 0
    for P in (1, 3, 17):
        for Hs in (1, 4):
            for iterations in (0, 1, 5):
                s = None if (P, Hs) == (3, 1) else np.ascontiguousarray(seeds[:P, :Hs])
                got = _both(clouds, pairs[:P], s, 2.5, iterations, 8, "n %d P %d H %d iterations %d" % (n, P, Hs, iterations), memo)
                ran += int((got[3] == 0).sum())
    assert ran > 100                                                          # the grid aligns clouds, it does not only flag them


def test_a_cloud_that_fills_the_lds():
    clouds = _moved_clouds(3, 4096, count=3, noise=0.01)
    got = _both(clouds, [[0, 1], [2, 0]], _seeds_for(3, 2, 2), 1.0, 2, 32, "n 4096")
    assert got[3].tolist() == [0, 0] and (got[2][:, 1] > 2048).all()


def _lattice(side=4):
    g = np.arange(side) - (side - 1) / 2.0
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def test_ties_go_to_the_lower_row_and_the_lower_seed():
    cube = _lattice()                                                         # 64 points, symmetric about the origin
    target = np.concatenate([cube, cube])                                     # every row twice: rows j and j + 64 tie
    source = np.concatenate([cube, np.full((64, 3), np.nan, np.float32)])
    clouds = np.stack([source, target, np.concatenate([cube + np.float32(0.5), cube + np.float32(0.5)])])
    shift = lambda x: R.pose_of(t=(x, 0.0, 0.0))
    # +1 and -1 along x: 48 exact matches each, sum d2 = 0 each: the lower seed; the identity comes last and wins on the count
    seeds = np.stack([shift(1.0), shift(-1.0), shift(-1.0), shift(1.0)])[None]
    got = _both(clouds, [[0, 1]], seeds[:, :2], 0.25, 0, 3, "two seeds tie")
    assert got[2].tolist() == [[0, 48, 64, 128]] and got[1][0].tolist() == [0.0, 0.75]
    got = _both(clouds, [[0, 1]], np.ascontiguousarray(seeds[:, 2:]), 0.25, 0, 3, "two seeds tie, the other order")
    assert got[2][0, 0] == 0 and got[0][0, 3] == -1.0
    got = _both(clouds, [[0, 1]], np.concatenate([seeds, shift(0.0)[None, None]], 1), 0.25, 3, 3, "the identity wins on the count")
    assert got[2].tolist() == [[4, 64, 64, 128]] and got[0][0].tolist() == R.IDENTITY.tolist()
    # every source row half a cell from eight target rows, each of them twice: sixteen equal d2, the lowest row -- in the restatement and
    # on the device alike; the refinement then walks on the ties' choice
    for iterations in (0, 1, 4):
        _both(clouds, [[0, 2], [2, 0], [1, 2]], None, 1.0, iterations, 3, "half-cell ties, iterations %d" % iterations)


def test_absent_rows_and_flags():
    n = 288
    clouds = _moved_clouds(11, n, count=5)
    clouds[1, 5::7] = np.nan                                                  # absent rows in a source ...
    clouds[2, 3::5, 1] = np.inf                                               # ... and in a target: one non-finite word is enough
    clouds[3] = np.nan                                                        # an all-absent cloud
    clouds[4, 20:] = np.nan                                                   # 20 rows: fewer than min_pairs
    pairs = [[1, 2], [2, 1], [0, 3], [3, 0], [0, 4], [4, 0], [-1, 0], [0, 5], [0, -1], [5, 5], [0, 0], [2, 2], [0, 1]]
    seeds = _seeds_for(11, len(pairs), 3)
    memo = {}
    got = _both(clouds, pairs, seeds, 2.5, 4, 32, "absent rows and flags", memo)
    pose, fit, info, status = got
    assert status[[0, 1]].tolist() == [0, 0] and status[[2, 3, 5]].tolist() == [512] * 3 and status[6:].tolist() == [256] * 4 + [0] * 3
    assert info[0, 2:].tolist() == [n - len(range(5, n, 7)), n - len(range(3, n, 5))] and info[2, 2:].tolist() == [n, 0]
    flagged = [2, 3, 5, 6, 7, 8, 9]
    assert info[6:10].tolist() == [[-1, 0, 0, 0]] * 4 and np.isnan(pose[flagged]).all() and np.isnan(fit[flagged]).all()
    assert fit[10].tolist() == [0.0, 1.0] and info[10, 1] == n                 # source == target cloud: every row finds itself
    # a gate below every distance
    got = _both(clouds, [[0, 1], [1, 0]], None, 1e-4, 2, 3, "a gate below every distance")
    assert got[3].tolist() == [512, 512]
    # a non-finite seed among finite ones loses wherever it stands; all seeds non-finite is NO_PAIR
    s = seeds[:3].copy()
    s[0, 0, 4], s[1, 2, 11], s[2, 1, 0] = np.nan, np.inf, -np.inf
    s[2, 0], s[2, 2] = np.nan, np.nan
    got = _both(clouds, [[0, 1], [0, 1], [0, 1]], s, 2.5, 2, 32, "non-finite seeds")
    assert got[3].tolist() == [0, 0, 256] and got[2][0, 0] in (1, 2) and got[2][1, 0] in (0, 1) and got[2][2].tolist() == [-1, 0, n, n - len(range(5, n, 7))]


def _entry_args(dev, n=64, P=3, Hs=2):
    L = H.pkg("lib")
    need = L.lib().epcnet_pair_register_workspace_bytes(P, Hs, n)
    out = dict(pose=Guarded((P, 12), torch.float64, dev), fit=Guarded((P, 2), torch.float64, dev), info=Guarded((P, 4), torch.int32, dev),
               status=Guarded((P,), torch.int32, dev), workspace=Guarded((need,), torch.uint8, dev))
    hold = [_up(_moved_clouds(1, n, count=2), np.float32), _up([[0, 1]] * P, np.int32), _up(_seeds_for(1, P, Hs), np.float64)]
    good = dict(clouds=hold[0].data_ptr(), num_clouds=2, n=n, pairs=hold[1].data_ptr(), num_pairs=P, seeds=hold[2].data_ptr(), num_seeds=Hs,
                max_dist=1.0, iterations=2, min_pairs=8, pose=out["pose"].t.data_ptr(), fit=out["fit"].t.data_ptr(),
                info=out["info"].t.data_ptr(), status=out["status"].t.data_ptr(), workspace=out["workspace"].t.data_ptr(), workspace_bytes=need)
    return good, out, hold


def test_refusals_launch_nothing_and_write_nothing():
    L = H.pkg("lib")
    lib, dev = L.lib(), torch.device("cuda")
    good, out, hold = _entry_args(dev)
    order = list(good)
    stream = torch.cuda.current_stream().cuda_stream
    bad = [dict(clouds=None), dict(pairs=None), dict(pose=None), dict(fit=None), dict(info=None), dict(status=None), dict(workspace=None),
           dict(clouds=good["clouds"] + 4), dict(workspace=good["workspace"] + 8), dict(n=0), dict(n=16), dict(n=48), dict(n=4128),
           dict(num_clouds=0), dict(num_pairs=-1), dict(num_pairs=(1 << 20) + 1), dict(num_seeds=0), dict(num_seeds=65), dict(seeds=None),
           dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(iterations=-1),
           dict(iterations=65), dict(min_pairs=2), dict(min_pairs=65)]
    for change in bad:
        a = dict(good, **change)
        assert lib.epcnet_pair_register(*[a[k] for k in order], stream) == L.EPC_EINVAL, change
    assert lib.epcnet_pair_register(*[dict(good, workspace_bytes=good["workspace_bytes"] - 1)[k] for k in order], stream) == L.EPC_ENOMEM
    assert lib.epcnet_pair_register(*[dict(good, num_pairs=0)[k] for k in order], stream) == L.EPC_OK        # no pair: nothing to launch
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values())
    assert lib.epcnet_pair_register(*[good[k] for k in order], stream) == L.EPC_OK                           # and the same arguments run
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values()) and not any(out[k].untouched() for k in ("pose", "fit", "info", "status"))
    del hold


def test_two_runs_and_one_captured_graph_replayed_on_other_data():
    RT, L = H.pkg("retrieval"), H.pkg("lib")
    dev, n, P, Hs = torch.device("cuda"), 288, 5, 3
    a, b = _moved_clouds(21, n, count=4), _moved_clouds(22, n, count=4)
    b[2, ::3] = np.nan
    pairs_a, pairs_b = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [0, 2]], np.int32), np.array([[3, 1], [-1, 2], [2, 0], [1, 1], [0, 4]], np.int32)
    seeds_a, seeds_b = _seeds_for(21, P, Hs), _seeds_for(22, P, Hs)
    seeds_b[2, 1, 3] = np.nan
    clouds, pairs, seeds = _up(a, np.float32), _up(pairs_a, np.int32), _up(seeds_a, np.float64)
    first = [t.clone() for t in RT.register_pairs(clouds, pairs, seeds, max_dist=2.5, iterations=3, min_pairs=16)]
    again = RT.register_pairs(clouds, pairs, seeds, max_dist=2.5, iterations=3, min_pairs=16)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, again))
    want_a = R.register_reference(a, pairs_a, seeds_a, 2.5, 3, 16)
    _equal(tuple(t.cpu().numpy() for t in first), want_a, "eager")
    ws = torch.empty(L.lib().epcnet_pair_register_workspace_bytes(P, Hs, n), dtype=torch.uint8, device=dev)
    RT.register_pairs(clouds, pairs, seeds, max_dist=2.5, iterations=3, min_pairs=16, workspace=ws)      # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = RT.register_pairs(clouds, pairs, seeds, max_dist=2.5, iterations=3, min_pairs=16, workspace=ws)

    def replay(c, p, s):
        clouds.copy_(_up(c, np.float32))
        pairs.copy_(_up(p, np.int32))
        seeds.copy_(_up(s, np.float64))
        g.replay()
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in out)

    want_b = R.register_reference(b, pairs_b, seeds_b, 2.5, 3, 16)
    assert 0 in want_b[3] and 256 in want_b[3] and want_b[3].tolist() != want_a[3].tolist()
    _equal(replay(b, pairs_b, seeds_b), want_b, "replay on other clouds, pairs and seeds")
    _equal(replay(a, pairs_a, seeds_a), want_a, "the second replay, on the first data")


def test_python_entries():
    RT, L = H.pkg("retrieval"), H.pkg("lib")
    dev, n = torch.device("cuda"), 64
    c = _moved_clouds(31, n, count=4)
    clouds, pairs = _up(c, np.float32), _up([[0, 1], [2, 3]], np.int32)
    seeds = _up(_seeds_for(31, 2, 2), np.float64)
    pose, fit, info, status = RT.register_pairs(clouds, pairs, seeds, max_dist=2.5, iterations=2, min_pairs=8)
    assert pose.shape == (2, 12) and fit.shape == (2, 2) and info.shape == (2, 4) and status.shape == (2,)
    assert pose.dtype == fit.dtype == torch.float64 and info.dtype == status.dtype == torch.int32
    empty = RT.register_pairs(clouds, pairs[:0], None)
    assert [tuple(t.shape) for t in empty] == [(0, 12), (0, 2), (0, 4), (0,)]
    for bad in (dict(clouds=clouds.cpu()), dict(clouds=clouds.double()), dict(clouds=clouds[:, :, [2, 1, 0]].transpose(0, 1)),
                dict(clouds=clouds[0]), dict(pairs=pairs.long()), dict(pairs=pairs.cpu()), dict(pairs=pairs.reshape(-1)),
                dict(seeds=seeds.float()), dict(seeds=seeds.cpu()), dict(seeds=seeds[:1]), dict(seeds=seeds.reshape(2, 24)),
                dict(workspace=torch.empty(64, dtype=torch.float32, device=dev))):
        with pytest.raises(L.EpcNetError):                                   # float32 seeds are refused, never converted
            RT.register_pairs(**dict(dict(clouds=clouds, pairs=pairs, seeds=seeds), **bad))
    with pytest.raises(L.EpcNetError):
        RT.register_pairs(clouds, pairs, seeds, iterations=65)
    # verify_revisits: the pairs (i, idx[i, j]) on the device, every output (Q, k, ...), a -1 flagged NO_PAIR
    idx = _up([[-1, -1, -1], [0, -1, -1], [1, 0, -1], [2, 0, 1]], np.int32)
    sub_pose = np.stack([R.pose_of(10.0 * i, 0, 0, (0.5 * i, 0, 0)) for i in range(4)])
    for kw in (dict(), dict(yaw=4), dict(sub_pose=_up(sub_pose, np.float64)), dict(sub_pose=_up(sub_pose, np.float64), yaw=2)):
        pose, fit, info, status = RT.verify_revisits(clouds, idx, max_dist=2.5, iterations=2, min_pairs=8, **kw)
        assert pose.shape == (4, 3, 12) and fit.shape == (4, 3, 2) and info.shape == (4, 3, 4) and status.shape == (4, 3)
        flagged = (idx < 0).cpu().numpy()
        assert (status.cpu().numpy()[flagged] == L.EPC_STATUS_NO_PAIR).all() and (status.cpu().numpy()[~flagged] & L.EPC_STATUS_NO_PAIR == 0).all()
        # the same as register_pairs on the pairs and seeds written out on the host
        hp = np.array([[i, j] for i, row in enumerate(idx.cpu().numpy()) for j in row], np.int32)
        if "sub_pose" in kw:                                                  # (seeds built with torch on the device: outside the bit contract)
            continue
        hs = RT.yaw_seeds(4, device=dev).unsqueeze(0).expand(len(hp), 4, 12).contiguous() if "yaw" in kw else None
        flat = RT.register_pairs(clouds, _up(hp, np.int32), hs, max_dist=2.5, iterations=2, min_pairs=8)
        for x, y in zip((pose, fit, info, status), flat):
            assert torch.equal(x.reshape(y.shape).view(torch.int32), y.view(torch.int32))
    with pytest.raises(L.EpcNetError):
        RT.verify_revisits(clouds, idx.long())
    with pytest.raises(L.EpcNetError):
        RT.verify_revisits(clouds[:3], idx)                                   # more queries than clouds


def _world(seed=41):
    """A static street 24 m long that no two places of look alike: ground, two walls with niches, posts of different heights."""
    rng = np.random.default_rng(seed)
    g = rng.uniform([-4, -6, 0], [28, 6, 0], size=(9000, 3))
    left = rng.uniform([-4, 6, 0], [28, 6, 4], size=(6000, 3))
    left[:, 1] += 0.8 * np.sin(left[:, 0] * 0.9) + 0.5 * (np.floor(left[:, 0] / 3.0) % 2)
    right = rng.uniform([-4, -6, 0], [28, -6, 3], size=(6000, 3))
    right[:, 1] -= 0.6 * np.cos(right[:, 0] * 0.55) + 0.7 * (np.floor(right[:, 0] / 5.0) % 2)
    posts = []
    for x in np.arange(-3.0, 28.0, 2.3):
        h = 1.0 + 2.5 * rng.uniform()
        p = rng.uniform([-0.15, -0.15, 0], [0.15, 0.15, h], size=(300, 3)) + [x + rng.uniform(-0.5, 0.5), rng.uniform(-4, 4), 0]
        posts.append(p)
    return np.concatenate([g, left, right] + posts)


def test_drive_forward_trajectory_revisit_search_verify_revisits():
    """A small out-and-back drive through the engine: 40 scans 1 m apart, 20 out and 20 back, each the world's points within 9 m of the
    sensor; submaps of 2 m every 1 m; clouds=True, revisit_search, verify_revisits seeded by the odometry.  The device's answer equals the
    restatement's on the drive's clouds bit for bit; and every pair that IS a revisit by the poses (within 1.5 m) is aligned with the true
    relative pose -- which the exact odometry gives -- within twice the worst error the restatement itself attains on these pairs, run on
    the CPU inside the test, and within the bound the gate allows: the submaps' grid averages are resampled views, not rigid copies, so
    no pose better than a fraction of a cell can be asked of them.  Measured on an MI355X: 31 revisits among the search's candidates, the
    restatement's worst error 9.7e-3 rad and 0.44 m; 17 revisits by the poses, 1.4e-2 rad and 0.41 m (256 points per submap of a street
    whose walls constrain the along-track direction weakly)."""
    RT, L = H.pkg("retrieval"), H.pkg("lib")
    dev = torch.device("cuda")
    eng, _ = H.make_engine("epc-net-l", O.seeded_weights("epc-net-l", 0), dev, in_flight=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S, length, spacing, slots, n = 40, 2.0, 1.0, 44, 256
    poses = SR.identity_poses(S).reshape(S, 3, 4)
    poses[:, 0, 3] = np.minimum(np.arange(S), S - 1 - np.arange(S)).astype(np.float64)
    world = _world()
    rng = np.random.default_rng(43)
    scans = []
    for i in range(S):
        near = world[np.abs(world[:, 0] - poses[i, 0, 3]) < 9.0]
        scans.append((near[rng.choice(len(near), size=1500, replace=False)] - poses[i, :, 3]).astype(np.float32))
    points, offsets = SR.pack(scans)
    args = (up(points), up(offsets), up(poses.reshape(S, 12)))
    kw = dict(along=up(np.arange(S) * 1.0), num_points=n, submaps=dict(length=length, spacing=spacing, max_submaps=slots, out_rows=S * 1500 * 3))
    plain = eng.forward_trajectory(*args, **kw)
    desc, status, sub_pose, num_out, clouds = eng.forward_trajectory(*args, clouds=True, **kw)
    assert len(plain) == 4                                                    # without clouds=True: exactly what it returned before
    for x, y in zip(plain, (desc, status, sub_pose, num_out)):
        assert x.dtype == y.dtype and torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0))
    K = int(num_out[0])
    assert clouds.shape == (slots, n, 3) and clouds.dtype == torch.float32 and 30 <= K < slots
    assert bool(torch.isfinite(clouds[:K]).all()) and bool(torch.isnan(clouds[K:]).all())
    along = up(np.arange(slots) * spacing)
    _, idx, _ = RT.revisit_search(desc, along, 3 * length, 5)
    sp, cl = sub_pose.cpu().numpy(), clouds.cpu().numpy()
    # the revisits by the poses themselves: for every submap the nearest one at least 3 lengths behind it, if within 1.5 m
    by_pose = np.full((slots, 1), -1, np.int32)
    for i in range(K):
        cand = [j for j in range(K) if j * spacing <= i * spacing - 3 * length and abs(sp[i, 3] - sp[j, 3]) <= 1.5]
        if cand:
            by_pose[i, 0] = min(cand, key=lambda j: (abs(sp[i, 3] - sp[j, 3]), j))
    assert (by_pose >= 0).sum() >= 10

    def check(idx, what):
        k = idx.shape[1]
        got = RT.verify_revisits(clouds, idx, sub_pose=sub_pose, max_dist=1.0, iterations=8, min_pairs=32)
        pose, fit, info, status_v = (t.cpu().numpy() for t in got)
        assert pose.shape == (slots, k, 12) and fit.shape == (slots, k, 2) and info.shape == (slots, k, 4) and status_v.shape == (slots, k)
        idx_h = idx.cpu().numpy()
        assert ((idx_h < 0) == (status_v == L.EPC_STATUS_NO_PAIR)).all()
        # the restatement on the same clouds and pairs, the seeds written out on the host
        pairs = np.array([[i, j] for i in range(slots) for j in idx_h[i]], np.int32)
        seeds = np.stack([(np.vstack([R.invert_pose(sp[j]).reshape(3, 4), [0, 0, 0, 1]]) @ np.vstack([sp[i].reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12)
                          if j >= 0 else np.full(12, np.nan) for i, j in pairs])[:, None]
        on_dev = RT.register_pairs(clouds, up(pairs), up(seeds), max_dist=1.0, iterations=8, min_pairs=32)
        want = R.register_reference(cl, pairs, seeds, 1.0, 8, 32)
        _equal(tuple(t.cpu().numpy() for t in on_dev), want, what)
        worst_ref, errors = np.zeros(2), []
        for row, (i, j) in enumerate(pairs):
            if j < 0 or np.linalg.norm(sp[i, [3, 7, 11]] - sp[j, [3, 7, 11]]) > 1.5:
                continue
            true = seeds[row, 0]                                              # exact odometry: the true relative pose
            assert want[3][row] == 0 and status_v[i, row % k] == 0 and fit[i, row % k, 1] > 0.5
            worst_ref = np.maximum(worst_ref, R.pose_error(want[0][row], true))
            errors.append(R.pose_error(pose[i, row % k], true))
        print("%s: %d revisits, the restatement's worst error %.3e rad %.3e m" % (what, len(errors), worst_ref[0], worst_ref[1]))
        for rot, trans in errors:
            assert rot <= 2 * worst_ref[0] and trans <= 2 * worst_ref[1]
            assert rot < 0.1 and trans < 0.5                                  # inside the gate: half of max_dist, a few degrees
        return len(errors)

    check(idx, "the search's candidates")
    assert check(up(by_pose), "the revisits by the poses") >= 10


def _bits_equal(a, b):
    view = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def test_engine_clouds_option_on_both_trajectory_entries():
    """clouds=True appends the metric clouds -- ops.grid_downsample(normalize=False) of the rows that fed the network, ground removed
    where the network's was -- and changes nothing else; the default returns exactly what it returned."""
    import stamps_ref as ST
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    eng, _ = H.make_engine("epc-net-l", O.seeded_weights("epc-net-l", 0), dev, in_flight=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ms = 1_000_000
    pose_time, pose = ST.odometry(21, 400, jitter_ns=200_000, wobble=0.01)       # 60 scans of 200 rows 50 ms apart over 4 s of odometry
    points, offsets = SR.pack([SR.scan(300 + i, 200, extent=12.0) for i in range(60)])
    scan_time = pose_time[10:310:5].copy() + 3 * ms
    dt = np.sort(np.random.default_rng(8).integers(0, 40 * ms, size=(60, 200)), axis=1).reshape(-1).astype(np.int32)
    points, offsets, scan_time, pose_time, pose, dt = (up(a) for a in (points, offsets, scan_time, pose_time, pose, dt))
    sub = dict(length=3.0, spacing=1.3, max_submaps=24, out_rows=4 * 60 * 200, max_range=50.0)
    moved, scan_pose, scan_status = ops.deskew_scans(points, offsets, scan_time, pose_time, pose, point_dt=dt)
    built = ops.build_submaps(moved, offsets, scan_pose, along=ops.travel_along(scan_pose, scan_status), **sub)
    for ground in (None, True):
        rows = built[0] if ground is None else ops.remove_ground(built[0], built[1])[0]
        want = ops.grid_downsample(rows, built[1], 32, normalize=False)[0].clone()
        plain = tuple(t.clone() for t in eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=dt, num_points=32, submaps=sub,
                                                              ground=ground))
        got = eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=dt, num_points=32, submaps=sub, ground=ground, clouds=True)
        assert len(plain) == 5 and len(got) == 6 and all(_bits_equal(x, y) for x, y in zip(plain, got)) and _bits_equal(got[5], want)
        assert got[5].shape == (24, 32, 3) and int(torch.isfinite(got[5]).all(2).all(1).sum()) >= int(got[3][0]) - 1
        plain = tuple(t.clone() for t in eng.forward_trajectory(moved, offsets, scan_pose, num_points=32, submaps=sub, ground=ground))
        got = eng.forward_trajectory(moved, offsets, scan_pose, num_points=32, submaps=sub, ground=ground, clouds=True)
        assert len(plain) == 4 and len(got) == 5 and all(_bits_equal(x, y) for x, y in zip(plain, got)) and got[4].shape == (24, 32, 3)


def test_no_pair_with_the_callers_workspace_and_with_none():
    """P = 0 pairs over two clouds of n = 32, with no seeds and with empty ones: the empty pairs, seeds and outputs have no address, the
    workspace's stands in for them -- the caller's, which nothing writes, or the entry's own."""
    RT = H.pkg("retrieval")
    dev = torch.device("cuda")
    clouds = _up(_moved_clouds(7, 32, count=2), np.float32)
    pairs = torch.empty((0, 2), dtype=torch.int32, device=dev)
    for ws in (torch.full((64,), 0xFF, dtype=torch.uint8, device=dev), None):
        for seeds in (None, torch.empty((0, 2, 12), dtype=torch.float64, device=dev)):
            out = RT.register_pairs(clouds, pairs, seeds, workspace=ws)
            torch.cuda.synchronize()
            assert [tuple(t.shape) for t in out] == [(0, 12), (0, 2), (0, 4), (0,)]
            assert [t.dtype for t in out] == [torch.float64, torch.float64, torch.int32, torch.int32]
            assert ws is None or bool((ws == 0xFF).all())
