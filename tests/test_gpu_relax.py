"""epcnet_trajectory_relax on the device against tests/relax_ref.py, the numpy restatement of include/epcnet_trajectory.h -- never the entry
under test.  Every output goes into a poisoned buffer with guard bytes in front of it and behind it, the workspace is exactly the size
asked for and full of 0xFF bytes, and all five outputs are compared on BIT PATTERNS: the definition fixes every rounding and every order
of summation, so there is no tolerance anywhere.  The grid of T x L around the wave, the scan block and the second scan level, the
special loops, every skip reason, a NaN pose in the middle, the scene of tests/test_relax_cpu.py, a captured graph replayed on other
data, two runs on a dirty workspace, and the Python entries."""
import numpy as np
import pytest
import torch

import helpers as H
import relax_ref as R
from helpers import Guarded

pytestmark = pytest.mark.gpu


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to("cuda")


def _raw(poses, pairs, rel, weights, odo=(1.0, 100.0), iterations=2, cg=8):
    """The entry itself on guarded, poisoned outputs and a guarded, poisoned workspace of exactly the size asked for."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    T, nl = len(poses), len(pairs)
    need = L.lib().epcnet_trajectory_relax_workspace_bytes(T, nl)
    assert need > 0 and need % 16 == 0
    out, cost = Guarded((T, 12), torch.float64, dev), Guarded((iterations + 1,), torch.float64, dev)
    chi2, status, num = Guarded((nl,), torch.float64, dev), Guarded((nl,), torch.int32, dev), Guarded((2,), torch.int32, dev)
    ws = Guarded((need,), torch.uint8, dev)
    arg = lambda t: t if t.numel() else ws.t.data_ptr()
    L.run.epcnet_trajectory_relax(_up(poses, np.float64), T, arg(_up(pairs, np.int32)), arg(_up(rel, np.float64)), arg(_up(weights, np.float64)),
                                  nl, float(odo[0]), float(odo[1]), iterations, cg, out.t, cost.t, arg(chi2.t), arg(status.t), num.t, ws.t, need)
    torch.cuda.synchronize()
    for g in (out, cost, chi2, status, num, ws):
        assert g.intact()
    return tuple(g.t.cpu().numpy() for g in (out, cost, chi2, status, num))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _equal(got, want, what):
    gp, gc, gx, gs, gn = got
    wp, wc, wx, ws, wn = want
    assert gn.tolist() == wn.tolist(), (what, "num_out", gn, wn)
    assert gs.tolist() == ws.tolist(), (what, "loop_status")
    assert (_bits(gc) == _bits(wc)).all(), (what, "cost", gc.tolist(), wc.tolist())
    assert (_bits(gx) == _bits(wx)).all(), (what, "loop_chi2", gx.tolist(), wx.tolist())
    bad = np.nonzero((_bits(gp) != _bits(wp)).any(1))[0]
    assert bad.size == 0, (what, "poses_out: %d nodes differ, the first is %d: %s / %s" % (bad.size, bad[0], gp[bad[0]].tolist(), wp[bad[0]].tolist()))


def _both(poses, pairs, rel, weights, what, odo=(1.0, 100.0), iterations=2, cg=8):
    want = R.relax_reference(poses, pairs, rel, weights, odo[0], odo[1], iterations, cg)
    got = _raw(poses, np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(rel, np.float64).reshape(-1, 12),
               np.asarray(weights, np.float64).reshape(-1, 2), odo, iterations, cg)
    _equal(got, want, what)
    return got


@pytest.mark.parametrize("T", [2, 63, 64, 65, 255, 256, 257, 513])
def test_grid_of_sizes(T):
    """L in {0, 1, 3, 17}, iterations 2, cg_iterations 8: around the wave, the scan block of 256 and the second scan level."""
    for nl in (0, 1, 3, 17):
        odo, pairs, rel, weights = R.walk_scene(T, nl, seed=T)
        got = _both(odo, pairs, rel, weights, "T %d L %d" % (T, nl))
        assert got[4].tolist() == [T, nl]
        if nl:
            assert np.isfinite(got[0]).all() and got[1][-1] < got[1][0]       # the grid relaxes trajectories, it does not only copy them
        else:
            assert (_bits(got[0]) == _bits(odo)).all() and (_bits(got[1]) == 0).all()


def _special(T=300, seed=5):
    """Loops of both directions, four ending on node 7 (and two more leaving it), one with w_t = 0 only, one with w_r = 0 only, two that
    close over the block boundary, and every skip reason."""
    odo, _, _, _ = R.walk_scene(T, 0, seed=seed)
    rng = np.random.default_rng(seed)
    pairs = [(200, 7), (150, 7), (7, 100), (260, 7), (7, 290), (90, 7),      # node 7 is an end of six loops; source < target among them
             (40, 41), (41, 40), (299, 0), (0, 299), (255, 256), (257, 3),
             (-1, 5), (5, T), (9, 9), (20, 30), (21, 31), (22, 32), (23, 33), (24, 34), (25, 35)]
    nl = len(pairs)
    rel = np.stack([R.compose(R.compose(R.inverse(odo[t % T]), odo[s % T]), R.pose_of(0.3 * rng.normal(size=3), 0.01 * rng.normal(size=3)))
                    for s, t in pairs])
    weights = np.tile(np.array([[1.0, 100.0]]), (nl, 1))
    weights[6] = (0.0, 50.0)                                                  # w_t = 0 only: used
    weights[7] = (2.0, 0.0)                                                   # w_r = 0 only: used
    skipped = list(range(12, 21))
    rel[15, 7] = np.nan                                                       # rel with a non-finite word
    rel[16, 3] = np.inf
    weights[17] = (np.nan, 1.0)
    weights[18] = (1.0, -1.0)                                                 # negative
    weights[19] = (0.0, 0.0)                                                  # both 0
    weights[20] = (np.inf, 1.0)
    return odo, np.array(pairs, np.int32), rel, weights, skipped


def test_special_loops_and_every_skip_reason():
    odo, pairs, rel, weights, skipped = _special()
    got = _both(odo, pairs, rel, weights, "special")
    want_status = [R.NO_EDGE if e in skipped else 0 for e in range(len(pairs))]
    assert got[3].tolist() == want_status and got[4].tolist() == [300, len(pairs) - len(skipped)]
    assert np.isnan(got[2][skipped]).all() and np.isfinite(np.delete(got[2], skipped)).all()
    assert got[1][-1] < got[1][0]


def test_a_nan_pose_in_the_middle():
    odo, pairs, rel, weights, _ = _special()
    odo = odo.copy()
    odo[140, 6] = np.nan
    odo[220] = np.nan
    got = _both(odo, pairs, rel, weights, "NaN at 140")
    assert got[4][0] == 140 and np.isnan(got[0][140:]).all() and np.isfinite(got[0][:140]).all()
    touching = [e for e, (s, t) in enumerate(pairs) if s >= 140 or t >= 140]
    assert touching and (got[3][touching] == R.NO_EDGE).all() and got[4][1] > 0
    # ... and at node 1 and node 0: T_eff < 2, nothing is solved and the finite poses come back as they are
    for first in (1, 0):
        broken = odo.copy()
        broken[first, 11] = np.inf
        got = _both(broken, pairs, rel, weights, "non-finite at %d" % first)
        assert got[4].tolist() == [first, 0] and (got[3] == R.NO_EDGE).all() and (_bits(got[1]) == 0).all()
        assert (_bits(got[0][:first]) == _bits(broken[:first])).all() and np.isnan(got[0][first:]).all()


def test_no_loop_used_is_a_bit_copy():
    odo, pairs, rel, weights = R.walk_scene(130, 5, seed=2)
    got = _both(odo, pairs, rel, np.zeros_like(weights), "zero weights", iterations=3)
    assert (_bits(got[0]) == _bits(odo)).all() and got[1].tolist() == [0.0] * 4 and (_bits(got[1]) == 0).all()
    assert np.isnan(got[2]).all() and (got[3] == R.NO_EDGE).all() and got[4].tolist() == [130, 0]


def test_a_failed_pivot_copies_the_input_through():
    """Odometry weights under which D overflows: a pivot is not > 0, the input comes back, every cost is +0.0 and num_out[1] is -1."""
    odo, pairs, rel, weights = R.walk_scene(300, 4, seed=6)
    got = _both(odo, pairs, rel, weights, "failed pivot", odo=(1e308, 1e308), iterations=2, cg=4)
    assert got[4].tolist() == [300, -1] and (_bits(got[0]) == _bits(odo)).all() and (_bits(got[1]) == 0).all()
    assert np.isnan(got[2]).all() and (got[3] == 0).all()


def test_iterations_zero_and_a_utm_origin():
    odo, pairs, rel, weights = R.walk_scene(70, 4, seed=3)
    odo = odo.copy()
    odo[:, 3] += 4.1e5
    odo[:, 7] += 5.5e6
    got = _both(odo, pairs, rel, weights, "iterations 0", iterations=0, cg=1)
    assert got[1].shape == (1,) and got[1][0] > 0 and np.abs(got[0] - odo).max() < 1e-8
    _both(odo, pairs, rel, weights, "utm", iterations=2, cg=30)


def test_the_scene_of_the_cpu_tests():
    _, odo, pairs, rel, weights = R.circle_scene()
    got = _both(odo, pairs, rel, weights, "circle", iterations=4, cg=36)
    assert got[1][-1] < 0.01 * got[1][0] and got[4].tolist() == [64, 3]


def test_two_runs_on_a_dirty_workspace_agree():
    """No memset and nothing left over: the second call on the workspace the first one used gives the same bits (and _raw's workspace is
    full of 0xFF to begin with)."""
    M = H.pkg("retrieval")
    L = H.pkg("lib")
    odo, pairs, rel, weights = R.walk_scene(257, 17, seed=8)
    args = (_up(odo, np.float64), _up(pairs, np.int32), _up(rel, np.float64), _up(weights, np.float64))
    ws = torch.full((L.lib().epcnet_trajectory_relax_workspace_bytes(257, 17),), 0xFF, dtype=torch.uint8, device="cuda")
    first = [t.cpu().numpy() for t in M.relax_trajectory(*args, iterations=2, cg_iterations=8, workspace=ws)]
    # another problem of the same size in between, so that the second run finds another call's leftovers
    other = R.walk_scene(257, 17, seed=9)
    M.relax_trajectory(_up(other[0], np.float64), _up(other[1], np.int32), _up(other[2], np.float64), _up(other[3], np.float64),
                       iterations=1, cg_iterations=3, workspace=ws)
    second = [t.cpu().numpy() for t in M.relax_trajectory(*args, iterations=2, cg_iterations=8, workspace=ws)]
    _equal(second, first, "second run")
    _equal(first, R.relax_reference(odo, pairs, rel, weights, 1.0, 100.0, 2, 8), "python entry")


def test_a_captured_graph_replays_on_other_poses_and_loops():
    M = H.pkg("retrieval")
    L = H.pkg("lib")
    T, nl = 257, 5
    scenes = [R.walk_scene(T, nl, seed=s) for s in (11, 12)]
    scenes[1][1][2] = (-1, 4)                                                  # the replay skips a loop the capture used ...
    nan_tail = scenes[1][0].copy()
    nan_tail[250:] = np.nan                                                    # ... and ends earlier
    scenes[1] = (nan_tail,) + tuple(scenes[1][1:])
    static = [_up(scenes[0][0], np.float64), _up(scenes[0][1], np.int32), _up(scenes[0][2], np.float64), _up(scenes[0][3], np.float64)]
    ws = torch.empty((L.lib().epcnet_trajectory_relax_workspace_bytes(T, nl),), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        M.relax_trajectory(*static, iterations=2, cg_iterations=6, workspace=ws)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = M.relax_trajectory(*static, iterations=2, cg_iterations=6, workspace=ws)
    for scene in (scenes[1], scenes[0], scenes[1]):
        for dst, src, dt in zip(static, scene, (np.float64, np.int32, np.float64, np.float64)):
            dst.copy_(_up(src, dt))
        graph.replay()
        torch.cuda.synchronize()
        _equal([t.cpu().numpy() for t in outs], R.relax_reference(*scene, 1.0, 100.0, 2, 6), "replay")
    assert int(outs[4][0]) == 250


def test_close_loops_equals_relax_trajectory_on_hand_built_arguments():
    """A synthetic verify_revisits result (Q, k) = (40, 2): unflagged good pairs, a -1 candidate, a flagged pair with a NaN pose, a low
    overlap and a high residual."""
    M = H.pkg("retrieval")
    T, Q, k = 48, 40, 2
    odo, _, _, _ = R.walk_scene(T, 0, seed=21)
    rng = np.random.default_rng(21)
    idx = np.full((Q, k), -1, np.int32)
    pose = np.full((Q, k, 12), np.nan)
    fit = np.full((Q, k, 2), np.nan)
    st = np.full((Q, k), 256, np.int32)
    want_w = np.zeros((Q, k, 2))
    for i, j, t, msr, overlap, flag in ((30, 0, 3, 0.01, 0.9, 0), (31, 1, 5, 0.02, 0.7, 0), (35, 0, 8, 0.2, 0.9, 0), (36, 0, 9, 0.01, 0.3, 0),
                                        (37, 1, 10, 0.01, 0.9, 512), (12, 0, 39, 0.03, 0.61, 0)):
        idx[i, j], st[i, j], fit[i, j] = t, flag, (msr, overlap)
        pose[i, j] = R.compose(R.compose(R.inverse(odo[t]), odo[i]), R.pose_of(0.2 * rng.normal(size=3), 0.01 * rng.normal(size=3)))
        if flag == 0 and msr <= 0.05 and overlap >= 0.6:
            want_w[i, j] = (2.0, 50.0)
    dev = [_up(odo, np.float64), _up(idx, np.int32), _up(pose, np.float64), _up(fit, np.float64), _up(st, np.int32)]
    got = M.close_loops(*dev, loop_weights=(2.0, 50.0), iterations=2, cg_iterations=20)
    src = np.repeat(np.arange(Q, dtype=np.int32), k)
    pairs = np.stack([src, idx.reshape(-1)], 1)
    hand = M.relax_trajectory(dev[0], _up(pairs, np.int32), _up(pose.reshape(-1, 12), np.float64), _up(want_w.reshape(-1, 2), np.float64),
                              iterations=2, cg_iterations=20)
    _equal([t.cpu().numpy() for t in got], [t.cpu().numpy() for t in hand], "close_loops")
    _equal([t.cpu().numpy() for t in got], R.relax_reference(odo, pairs, pose.reshape(-1, 12), want_w.reshape(-1, 2), 1.0, 100.0, 2, 20), "ref")
    assert got[4].tolist() == [T, 3] and int((got[3] == 0).sum()) == 3


def test_python_entry_refuses_what_it_would_have_to_convert():
    M = H.pkg("retrieval")
    L = H.pkg("lib")
    odo, pairs, rel, weights = R.walk_scene(20, 2, seed=1)
    good = [_up(odo, np.float64), _up(pairs, np.int32), _up(rel, np.float64), _up(weights, np.float64)]
    for i, bad in ((0, good[0].float()), (1, good[1].long()), (2, good[2].float()), (3, good[3].float()), (0, good[0].cpu()),
                   (2, good[2][:1]), (0, good[0].reshape(-1, 6))):
        args = list(good)
        args[i] = bad
        with pytest.raises(L.EpcNetError):
            M.relax_trajectory(*args)
    with pytest.raises(L.EpcNetError) as e:
        M.relax_trajectory(good[0].float(), *good[1:])
    assert "never converted" in str(e.value)
    with pytest.raises(L.EpcNetError) as e:                                   # the library's own refusals come through with their text
        M.relax_trajectory(*good, odo_weights=(0.0, 1.0))
    assert e.value.status == L.EPC_EINVAL and "odo_w_t" in str(e.value)
    with pytest.raises(L.EpcNetError) as e:
        M.relax_trajectory(*good, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    assert e.value.status == L.EPC_ENOMEM


def test_no_loop_on_two_poses_with_the_callers_workspace_and_with_none():
    """L = 0 loops on T = 2 poses through the Python entry: the empty pairs, rel, weights, chi2 and status have no address, the
    workspace's stands in for them -- the caller's or the entry's own -- and the poses come back bit for bit."""
    M, L = H.pkg("retrieval"), H.pkg("lib")
    odo, pairs, rel, weights = R.walk_scene(2, 0, seed=4)
    want = R.relax_reference(odo, pairs, rel, weights, 1.0, 100.0, 2, 8)
    args = (_up(odo, np.float64), _up(np.zeros((0, 2)), np.int32), _up(np.zeros((0, 12)), np.float64), _up(np.zeros((0, 2)), np.float64))
    for ws in (torch.full((L.lib().epcnet_trajectory_relax_workspace_bytes(2, 0),), 0xFF, dtype=torch.uint8, device="cuda"), None):
        got = [t.cpu().numpy() for t in M.relax_trajectory(*args, iterations=2, cg_iterations=8, workspace=ws)]
        _equal(got, want, "L = 0, workspace %s" % ("given" if ws is not None else "None"))
        assert (_bits(got[0]) == _bits(odo)).all() and (_bits(got[1]) == 0).all() and got[4].tolist() == [2, 0]
        assert got[2].shape == (0,) and got[3].shape == (0,)
