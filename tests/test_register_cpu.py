"""The definition of include/epcnet_pairs.h as tests/register_ref.py restates it, without a device: the seventh header's binding, the
restatement's Jacobi against numpy.linalg.eigh, its tree sum against math.fsum, the recovery of an exact rigid motion on structured
scenes, the choice among yaw seeds, absent rows, the flags, and the entry's refusals, which launch nothing."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import helpers as H
import register_ref as R

N = 512
# twice the worst errors the restatement attains on the scenes below, run on the CPU (test_exact_rigid_motion_is_recovered prints them)
ROT_TOL, TRANS_TOL = 2 * 1.6e-9, 2 * 2.7e-8


def _scene_pair(seed, true, n=N):
    """(clouds (2, n, 3) float32: source, target) with source = inv(true)(target) before the rounding to float32."""
    tgt = R.structured_scene(seed, n)
    return np.stack([R.apply_pose(R.invert_pose(true), tgt).astype(np.float32), tgt.astype(np.float32)])


def test_seventh_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_pairs.h")).read()
    assert L.PAIRS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_pairs.h")
    functions, constants, status = L.parse_header(text, need_status=False, scalars=L._REVISIT_SCALARS)
    assert list(functions) == L.PAIR_EXPORTS == ["epcnet_pair_register_workspace_bytes", "epcnet_pair_register"]
    assert status == {} and constants == {"EPC_STATUS_NO_PAIR": 256, "EPC_STATUS_NO_FIT": 512}
    assert L.EPC_STATUS_NO_PAIR == R.NO_PAIR == 256 and L.EPC_STATUS_NO_FIT == R.NO_FIT == 512
    taken = [v for k, v in L._constants.items() if k.startswith("EPC_STATUS_") and k not in constants]
    assert not any(v & (256 | 512) for v in taken)                            # the bits 1 .. 128 are the earlier headers'
    with pytest.raises(ValueError):                                           # a `double` by value needs the scalars that allow it
        L.parse_header(text, need_status=False)
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.REVISIT_EXPORTS, L.LAUNCHING):
        assert not set(L.PAIR_EXPORTS) & set(other)
    for name in L.PAIR_EXPORTS:
        assert hasattr(L.lib(), name)
    size, entry = L.lib().epcnet_pair_register_workspace_bytes, L.lib().epcnet_pair_register
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int] * 3
    ret, types, names = functions["epcnet_pair_register"]
    assert names == ["clouds", "num_clouds", "n", "pairs", "num_pairs", "seeds", "num_seeds", "max_dist", "iterations", "min_pairs", "pose",
                     "fit", "info", "status", "workspace", "workspace_bytes", "stream"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and entry.restype is ctypes.c_int
    assert types[names.index("clouds")] == "float*" and types[names.index("pairs")] == types[names.index("info")] == "int32_t*"
    assert types[names.index("seeds")] == types[names.index("pose")] == types[names.index("fit")] == "double*"
    assert types[names.index("max_dist")] == "double"
    P, i = ctypes.c_void_p, ctypes.c_int
    assert entry.argtypes == [P, i, i, P, i, P, i, ctypes.c_double, i, i, P, P, P, P, P, ctypes.c_size_t, P]
    assert hasattr(L.run, "epcnet_pair_register") and not hasattr(L.run, "epcnet_pair_register_workspace_bytes")

    class Fake:
        def __init__(self, dtype):
            self.dtype, self.is_cuda = dtype, True

        def data_ptr(self):
            return 0x10000

    f32, f64, i32 = Fake(torch.float32), Fake(torch.float64), Fake(torch.int32)
    with pytest.raises(L.EpcNetError) as e:                                   # float32 seeds are refused before the library is reached
        L.run.epcnet_pair_register(f32, 2, 64, i32, 1, f32, 1, 1.0, 4, 32, f64, f64, i32, i32, None, 0, stream=0)
    assert "argument 6" in str(e.value) and "seeds" in str(e.value) and "torch.float64" in str(e.value)
    with pytest.raises(L.EpcNetError) as e:                                   # everything typed right, an int for the double: the null workspace
        L.run.epcnet_pair_register(f32, 2, 64, i32, 1, None, 1, 1, 4, 32, f64, f64, i32, i32, None, 0, stream=0)
    assert e.value.status == L.EPC_EINVAL and "epcnet_pair_register: null pointer" in str(e.value)


def test_jacobi_agrees_with_eigh():
    """Random symmetric 4x4 matrices, among them ones with repeated and zero eigenvalues: the eigenvalues and the residual |N v - l v| of
    the dominant pair against numpy.linalg.eigh, within 8 times the error eigh itself shows (its residual and its departure from the
    spectrum the matrix was built from), floored at 8 ulp of the matrix's norm."""
    rng = np.random.default_rng(1)
    for trial in range(200):
        Q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        ev = [rng.normal(size=4) * 10.0 ** rng.integers(-3, 4), np.array([3.0, 3.0, 1.0, -2.0]), np.array([0.0, 0.0, 0.0, 5.0]),
              np.array([2.0, 2.0, 2.0, 2.0]), np.array([1.0, 0.0, 0.0, -1.0])][trial % 5]
        N = (Q * ev) @ Q.T
        N = (N + N.T) / 2
        scale = max(float(np.abs(N).max()), 1e-300)
        lam, vec = np.linalg.eigh(N)
        eigh_err = max(float(np.abs(N @ vec - vec * lam).max()), float(np.abs(lam - np.sort(ev)).max()))
        margin = 8 * max(eigh_err, np.finfo(np.float64).eps * scale)
        A, V = R.jacobi(N.tolist())
        A, V = np.array(A), np.array(V)
        assert np.abs(np.sort(np.diag(A)) - lam).max() <= margin, trial
        assert np.abs(A - np.diag(np.diag(A))).max() <= margin, trial          # what is left beside the diagonal
        assert np.abs(V.T @ V - np.eye(4)).max() <= 64 * np.finfo(np.float64).eps, trial
        q = np.array(R.dominant(A.tolist(), V.tolist()))
        assert np.abs(N @ q - lam[-1] * q).max() <= margin, trial


def test_sweep_count_settles_the_rotation():
    """One more sweep than the header's count moves no bit of the rotation on the Horn matrices of noisy point sets."""
    rng = np.random.default_rng(2)
    for trial in range(200):
        s = rng.normal(size=(40, 3)) * rng.uniform(0.1, 30, size=3)
        q = R.apply_pose(R.pose_of(rng.uniform(-180, 180), rng.uniform(-30, 30), rng.uniform(-30, 30), rng.normal(size=3)), s)
        q += 0.05 * rng.normal(size=q.shape)
        sums = np.concatenate([[40.0], s.sum(0), q.sum(0), (s.T @ q).reshape(9), [0.0]])
        N = R.horn_matrix(sums)
        assert R.rotation_of(R.dominant(*R.jacobi(N, R.SWEEPS))) == R.rotation_of(R.dominant(*R.jacobi(N, R.SWEEPS + 1))), trial


def test_tree_sum_agrees_with_fsum():
    rng = np.random.default_rng(3)
    for scale in (1.0, 1e6):
        v = (rng.normal(size=(17, R.LEAVES)) * scale).astype(np.float32).astype(np.float64)
        v[:, 3000:] = 0.0                                                      # the padding of a cloud shorter than the tree
        got = R.tree_sum(v)
        for k in range(17):
            exact = math.fsum(v[k])
            # pairwise summation over 2^12 leaves: 12 roundings deep, each at most half an ulp of a partial sum <= sum |v|
            assert abs(got[k] - exact) <= 12 * 0.5 * np.finfo(np.float64).eps * np.abs(v[k]).sum()
            assert abs(got[k] - exact) <= 4 * np.spacing(np.abs(v[k]).sum())   # "a few ulps" of the sum of magnitudes
    assert R.tree_sum(np.ones(R.LEAVES)) == R.LEAVES and R.tree_sum(np.zeros(R.LEAVES)) == 0.0
    assert np.signbit(R.tree_sum(np.full(R.LEAVES, -0.0))) and not np.signbit(R.tree_sum(np.r_[np.full(8, -0.0), np.zeros(R.LEAVES - 8)]))


def test_exact_rigid_motion_is_recovered():
    """20 degrees of yaw, 5 of pitch and 2 m on three structured scenes of 512 rows, from two seeds inside the basin (3 degrees / 0.4 m and
    4.6 degrees / 0.5 m off).  The restatement attains, on the CPU: rotation error at most 1.6e-9 rad, translation error at most 2.7e-8 m
    (float32 rows of a scene 40 m across: the rounding of the source cloud); the test asserts twice those.  The 135 degree turn of the next
    test attains 8.2e-10 rad and 1.3e-8 m and is held to the same bound."""
    true = R.pose_of(20, 5, 0, (1.6, -1.0, 0.663))
    assert abs(np.linalg.norm(true.reshape(3, 4)[:, 3]) - 2.0) < 1e-3
    worst = [0.0, 0.0]
    for scene in range(3):
        clouds = _scene_pair(scene, true)
        for seed in (R.pose_of(17, 3, 0, (1.3, -0.8, 0.5)), R.pose_of(24, 7, 1, (2.0, -1.3, 0.9))):
            before = R.pose_error(seed, true)
            assert before[0] > 0.05 and before[1] > 0.3
            pose, fit, info, status = R.register_reference(clouds, [[0, 1]], seed[None, None], 1.0, 16, 32)
            assert status.tolist() == [0] and info.tolist() == [[0, N, N, N]]
            assert fit[0, 1] == 1.0 and 0.0 <= fit[0, 0] < 1e-10
            rot, trans = R.pose_error(pose[0], true)
            worst = [max(worst[0], rot), max(worst[1], trans)]
            print("scene %d: rotation error %.3e rad, translation error %.3e m" % (scene, rot, trans))
            assert rot <= ROT_TOL and trans <= TRANS_TOL
            R_ = pose[0].reshape(3, 4)[:, :3]
            assert np.abs(R_ @ R_.T - np.eye(3)).max() < 1e-14                 # a rotation, from the unnormalised quaternion
    print("worst: %.3e rad, %.3e m" % tuple(worst))


def test_the_right_yaw_seed_is_chosen_for_a_135_degree_turn():
    true = R.pose_of(135, 0, 0, (0.5, 0.3, 0.0))
    clouds = _scene_pair(5, true)
    seeds = np.stack([R.pose_of(45.0 * m) for m in range(8)])[None]
    pose, fit, info, status = R.register_reference(clouds, [[0, 1]], seeds, 1.0, 16, 32)
    assert status.tolist() == [0] and info.tolist() == [[3, N, N, N]]
    rot, trans = R.pose_error(pose[0], true)
    print("135 degrees: rotation error %.3e rad, translation error %.3e m" % (rot, trans))
    assert rot <= ROT_TOL and trans <= TRANS_TOL
    # a non-finite seed loses to every finite one, whatever its position; with iterations 0 the pose is the seed's own words
    seeds[0, 0, 5] = np.nan
    seeds[0, 7, 11] = np.inf
    pose0, _, info0, status0 = R.register_reference(clouds, [[0, 1]], seeds, 1.0, 0, 32)
    assert status0.tolist() == [0] and info0[0, 0] == 3 and pose0[0].tobytes() == seeds[0, 3].tobytes()


def test_absent_rows_change_nothing_but_the_counts():
    true = R.pose_of(20, 5, 0, (1.6, -1.0, 0.663))
    seed = R.pose_of(17, 3, 0, (1.3, -0.8, 0.5))[None, None]
    clouds = _scene_pair(7, true)
    want = R.register_reference(clouds, [[0, 1]], seed, 1.0, 8, 32)
    # absent rows behind the source and scattered through the target: the same points, the same order, the same tree -- the same bits
    wide = np.full((2, 2 * N, 3), np.nan, np.float32)
    wide[0, :N] = clouds[0]
    wide[1, ::2] = clouds[1]
    wide[1, 1::4, 0] = np.inf                                                  # one non-finite word makes a row absent
    wide[1, 1::4, 1:] = 0.0
    got = R.register_reference(wide, [[0, 1]], seed, 1.0, 8, 32)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[2].tolist() == want[2].tolist() == [[0, N, N, N]] and got[3].tolist() == [0]
    # rows taken away: the counts say so, the overlap is still whole, the motion is still found
    fewer = clouds.copy()
    fewer[0, 100:164] = np.nan
    fewer[1, 7::50, 2] = np.nan
    pose, fit, info, status = R.register_reference(fewer, [[0, 1]], seed, 1.0, 8, 32)
    nt = N - len(range(7, N, 50))
    assert status.tolist() == [0] and info[0, 2:].tolist() == [N - 64, nt] and info[0, 1] <= N - 64 and 0.9 < fit[0, 1] <= 1.0
    rot, trans = R.pose_error(pose[0], true)
    assert rot < 1e-3 and trans < 1e-2                                         # (some rows lost their partner: no longer an exact motion)


def test_flags():
    true = R.pose_of(5, 0, 0, (0.2, 0.0, 0.0))
    clouds = _scene_pair(8, true, 64)
    nan_seed = np.full((1, 1, 12), np.nan)
    for pairs, seeds, max_dist, min_pairs, bit, rows in (([[-1, 1]], None, 1.0, 3, R.NO_PAIR, [0, 0]), ([[0, 2]], None, 1.0, 3, R.NO_PAIR, [0, 0]),
                                                         ([[0, 1]], nan_seed, 1.0, 3, R.NO_PAIR, [64, 64]),
                                                         ([[0, 1]], None, 1e-6, 3, R.NO_FIT, [64, 64]), ([[0, 1]], None, 5.0, 3, 0, [64, 64])):
        pose, fit, info, status = R.register_reference(clouds, pairs, seeds, max_dist, 2, min_pairs)
        assert status.tolist() == [bit] and info[0, 2:].tolist() == rows
        if bit:
            assert np.isnan(pose).all() and np.isnan(fit).all() and info[0, :2].tolist() == [-1, 0]
    empty = clouds.copy()
    empty[1] = np.nan                                                          # an all-absent target
    assert R.register_reference(empty, [[0, 1]], None, 1.0, 2, 3)[3].tolist() == [R.NO_FIT]
    assert R.gate2_of(1e30) == R.F32_MAX and R.gate2_of(0.5) == np.float32(0.25)


def test_size_query_answers_zero_for_what_the_entry_refuses():
    size = H.pkg("lib").lib().epcnet_pair_register_workspace_bytes
    for good in ((1, 1, 32), (5, 8, 1024), (0, 1, 32), (1 << 20, 1, 32), (17, 64, 4096), (3, 4, 224)):
        assert size(*good) % 16 == 0 and (size(*good) > 0 or good[0] == 0), good
    for bad in ((-1, 1, 32), ((1 << 20) + 1, 1, 32), (5, 0, 32), (5, 65, 32), (5, 1, 0), (5, 1, 16), (5, 1, 48), (5, 1, 4128), (5, 1, -32)):
        assert size(*bad) == 0, bad
    assert size(5, 8, 1024) >= 5 * 8 * 4 * 17 * 8                             # 17 sums per pair, seed and chunk of 256 rows


def test_refusals_launch_nothing():
    """Every EPC_EINVAL and the EPC_ENOMEM are decided on the host before anything touches a device: the pointers here are made-up
    addresses that are never followed."""
    L = H.pkg("lib")
    lib = L.lib()
    A = 0x10000
    need = lib.epcnet_pair_register_workspace_bytes(5, 4, 256)
    good = dict(clouds=A, num_clouds=6, n=256, pairs=2 * A, num_pairs=5, seeds=3 * A, num_seeds=4, max_dist=1.0, iterations=5, min_pairs=32,
                pose=4 * A, fit=5 * A, info=6 * A, status=7 * A, workspace=8 * A, workspace_bytes=need)
    order = list(good)
    bad = [dict(clouds=None), dict(pairs=None), dict(pose=None), dict(fit=None), dict(info=None), dict(status=None), dict(workspace=None),
           dict(clouds=A + 4), dict(workspace=8 * A + 8), dict(n=0), dict(n=16), dict(n=48), dict(n=4128), dict(num_clouds=0), dict(num_pairs=-1),
           dict(num_pairs=(1 << 20) + 1), dict(num_seeds=0), dict(num_seeds=65), dict(seeds=None), dict(max_dist=0.0), dict(max_dist=-1.0),
           dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(iterations=-1), dict(iterations=65), dict(min_pairs=2),
           dict(min_pairs=257)]
    for change in bad:
        a = dict(good, **change)
        assert lib.epcnet_pair_register(*[a[k] for k in order], None) == L.EPC_EINVAL, change
        assert b"epcnet_pair_register" in lib.epc_last_error()
    assert lib.epcnet_pair_register(*[dict(good, workspace_bytes=need - 1)[k] for k in order], None) == L.EPC_ENOMEM
    assert lib.epcnet_pair_register(*[dict(good, num_pairs=0)[k] for k in order], None) == L.EPC_OK          # no pair: nothing to launch
    assert lib.epcnet_pair_register(*[dict(good, num_pairs=0, workspace_bytes=0)[k] for k in order], None) == L.EPC_OK


def test_python_entry_refuses_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L, RT = H.pkg("lib"), H.pkg("retrieval")
    with pytest.raises(L.EpcNetError):
        RT.register_pairs(torch.zeros(2, 32, 3), torch.zeros(1, 2, dtype=torch.int32))
    seeds = RT.yaw_seeds(8)                                                  # plain torch: runs anywhere
    assert seeds.shape == (8, 12) and seeds.dtype == torch.float64
    want = np.stack([R.pose_of(45.0 * m) for m in range(8)])
    assert np.abs(seeds.numpy() - want).max() < 1e-15 and seeds[0].tolist() == R.IDENTITY.tolist()
    base = torch.from_numpy(np.stack([R.pose_of(10, 2, 0, (1, 2, 3)), R.pose_of(-30, 0, 5, (0, 1, 0))]))
    both = RT.yaw_seeds(4, base).numpy()
    assert both.shape == (2, 4, 12)
    for b in range(2):
        for m in range(4):
            want = (np.vstack([base[b].numpy().reshape(3, 4), [0, 0, 0, 1]]) @ np.vstack([R.pose_of(90.0 * m).reshape(3, 4), [0, 0, 0, 1]]))[:3]
            assert np.abs(both[b, m].reshape(3, 4) - want).max() < 1e-15
