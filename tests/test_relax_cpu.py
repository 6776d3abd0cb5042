"""The definition of include/epcnet_trajectory.h as tests/relax_ref.py restates it, without a device: the ninth header's binding, the
Jacobian against finite differences, the structure the method rests on (the preconditioned matrix is I + rank 6 L), the minimiser against
scipy, the cost, the gauge, consistent loops, the rules, and the entry's refusals, which launch nothing."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers as H
import relax_ref as R

ODO = (1.0, 100.0)


@pytest.fixture(scope="module", autouse=True)
def _restatement_and_library_speak_of_one_header():
    """What every test here rests on: the status bit of the restatement is the one the built library's binding read from the header."""
    L = H.pkg("lib")
    assert L.EPC_STATUS_NO_EDGE == R.NO_EDGE and "epcnet_trajectory_relax" in L.TRAJECTORY_EXPORTS


@pytest.fixture(scope="module")
def scene():
    """T = 64 nodes on two laps of a circle with 10 m steps, seeded odometry noise, 3 exact loops from lap 2 to lap 1; relaxed once with
    iterations 4 and cg_iterations 36 = 12 L."""
    truth, odo, pairs, rel, weights = R.circle_scene()
    return dict(truth=truth, odo=odo, pairs=pairs, rel=rel, weights=weights, out=R.relax_reference(odo, pairs, rel, weights, *ODO, 4, 36))


def test_ninth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_trajectory.h")).read()
    assert L.TRAJECTORY_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_trajectory.h")
    functions, constants, status = L.parse_header(text, need_status=False, scalars=L._REVISIT_SCALARS)
    assert list(functions) == L.TRAJECTORY_EXPORTS == ["epcnet_trajectory_relax_workspace_bytes", "epcnet_trajectory_relax"]
    assert status == {} and constants == {"EPC_STATUS_NO_EDGE": 1024}
    assert L.EPC_STATUS_NO_EDGE == R.NO_EDGE == 1024
    taken = [v for k, v in L._constants.items() if k.startswith("EPC_STATUS_") and k not in constants]
    assert taken and not any(v & 1024 for v in taken) and max(taken) == 512    # the bits up to 512 are the earlier headers'
    with pytest.raises(ValueError):                                           # a `double` by value needs the scalars that allow it
        L.parse_header(text, need_status=False)
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.REVISIT_EXPORTS, L.PAIR_EXPORTS,
                  L.FORM_EXPORTS, L.LAUNCHING):
        assert not set(L.TRAJECTORY_EXPORTS) & set(other)
    for name in L.TRAJECTORY_EXPORTS:
        assert hasattr(L.lib(), name)
    size, entry = L.lib().epcnet_trajectory_relax_workspace_bytes, L.lib().epcnet_trajectory_relax
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int] * 2
    ret, types, names = functions["epcnet_trajectory_relax"]
    assert names == ["poses", "num_poses", "pairs", "rel", "weights", "num_loops", "odo_w_t", "odo_w_r", "iterations", "cg_iterations",
                     "poses_out", "cost", "loop_chi2", "loop_status", "num_out", "workspace", "workspace_bytes", "stream"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and entry.restype is ctypes.c_int
    for n in ("poses", "rel", "weights", "poses_out", "cost", "loop_chi2"):
        assert types[names.index(n)] == "double*"
    for n in ("pairs", "loop_status", "num_out"):
        assert types[names.index(n)] == "int32_t*"
    assert types[names.index("odo_w_t")] == types[names.index("odo_w_r")] == "double"
    P, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert entry.argtypes == [P, i, P, P, P, i, d, d, i, i, P, P, P, P, P, P, ctypes.c_size_t, P]
    assert hasattr(L.run, "epcnet_trajectory_relax") and not hasattr(L.run, "epcnet_trajectory_relax_workspace_bytes")

    class Fake:
        def __init__(self, dtype):
            self.dtype, self.is_cuda = dtype, True

        def data_ptr(self):
            return 0x10000

    f32, f64, i32 = Fake(torch.float32), Fake(torch.float64), Fake(torch.int32)
    with pytest.raises(L.EpcNetError) as e:                                   # float32 poses are refused before the library is reached
        L.run.epcnet_trajectory_relax(f32, 8, i32, f64, f64, 1, 1.0, 100.0, 1, 1, f64, f64, f64, i32, i32, f64, 1 << 20, stream=0)
    assert "argument 1" in str(e.value) and "poses" in str(e.value) and "torch.float64" in str(e.value)
    # a second declaration of a name, in this header or against an earlier one, is refused like everywhere
    with pytest.raises(ValueError):
        L.parse_header(text + "\nint epcnet_trajectory_relax(int n);\n", need_status=False, scalars=L._REVISIT_SCALARS)


def test_entry_refusals_launch_nothing():
    """EPC_EINVAL / EPC_ENOMEM from addresses that are never followed: nothing is launched, so no device is needed."""
    L = H.pkg("lib")
    size = L.lib().epcnet_trajectory_relax_workspace_bytes
    assert size(64, 3) > 0 and size(64, 3) % 16 == 0 and size(64, 4) > size(64, 3) and size(65, 3) > size(64, 3)
    for T, nl in ((1, 0), (65537, 0), (64, -1), (64, (1 << 20) + 1)):
        assert size(T, nl) == 0
    assert size(2, 0) > 0 and size(65536, 1 << 20) > 0
    a = 0x10000

    def call(T=64, nl=3, poses=a, pairs=a, rel=a, weights=a, wt=1.0, wr=100.0, it=4, cg=36, out=a, cost=a, chi2=a, status=a, num=a, ws=a,
             ws_bytes=None):
        need = size(T, nl) if ws_bytes is None else ws_bytes
        return L.lib().epcnet_trajectory_relax(poses, T, pairs, rel, weights, nl, wt, wr, it, cg, out, cost, chi2, status, num, ws, need, None)

    bad = [dict(T=1), dict(T=65537), dict(nl=-1), dict(nl=(1 << 20) + 1), dict(it=-1), dict(it=65), dict(cg=0), dict(cg=4097),
           dict(wt=0.0), dict(wr=-1.0), dict(wt=float("nan")), dict(wr=float("inf")), dict(ws=a + 8),
           dict(poses=None), dict(pairs=None), dict(rel=None), dict(weights=None), dict(out=None), dict(cost=None), dict(chi2=None),
           dict(status=None), dict(num=None), dict(ws=None)]
    for kw in bad:
        assert call(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_trajectory_relax" in L.lib().epc_last_error()
    assert call(ws_bytes=size(64, 3) - 1) == L.EPC_ENOMEM and call(T=2, nl=0, pairs=None, rel=None, weights=None, ws_bytes=0) == L.EPC_ENOMEM


def _dense_jacobian(A, B, C):
    J = np.zeros((6, 6))
    J[:3, :3], J[:3, 3:], J[3:, 3:] = A, B, C
    return J


def test_jacobian_agrees_with_finite_differences():
    """J against (r(retract(b, h e_k)) - r) / h and -J against the same on node a (the residual depends on eta_b - eta_a alone to first
    order), h = 1e-6, on 20 random edges with translations of metres and rotations up to a radian.  Measured: 6.5e-6, the second-order
    term h |r''| / 2 of a one-sided difference; the bound is 10 times that."""
    rng = np.random.default_rng(1)
    rnd = lambda: R.pose_of(rng.normal(size=3) * 5, rng.normal(size=3) * 0.7).reshape(1, 3, 4)
    h, worst = 1e-6, 0.0
    for _ in range(20):
        Xa, Xb, Z = rnd(), rnd(), rnd()
        Ra, Rb, ca, cb = Xa[:, :, :3].copy(), Xb[:, :, :3].copy(), Xa[:, :, 3].copy(), Xb[:, :, 3].copy()
        ZR, zt = Z[:, :, :3].copy(), Z[:, :, 3].copy()
        A, B, C, _, _ = R.linearise(Ra, Rb, ca, cb, ZR, zt, np.ones(1), np.ones(1))
        J = _dense_jacobian(A[0], B[0], C[0])
        r0 = np.concatenate(R.residual(Ra, Rb, ca, cb, ZR, zt)[:2], 1)[0]
        for k in range(6):
            e = np.zeros((1, 6))
            e[0, k] = h
            Rb2, cb2 = R.retract(Rb, cb, e)
            worst = max(worst, np.abs((np.concatenate(R.residual(Ra, Rb2, ca, cb2, ZR, zt)[:2], 1)[0] - r0) / h - J[:, k]).max())
            Ra2, ca2 = R.retract(Ra, ca, e)
            worst = max(worst, np.abs((np.concatenate(R.residual(Ra2, Rb, ca2, cb, ZR, zt)[:2], 1)[0] - r0) / h + J[:, k]).max())
    print("Jacobian against finite differences: %.3e" % worst)
    assert worst <= 6.5e-5


def _dense_problem(P):
    """Of a linearised Problem: (S^T H S, blockdiag(D_n)) in the increments of nodes 1 .. te - 1, built with numpy's own matrix products
    from the edges' J -- not with the restatement's product."""
    te = P.te

    def blocks(J, wt, wr):
        Jf = np.zeros((len(J[0]), 6, 6))
        Jf[:, :3, :3], Jf[:, :3, 3:], Jf[:, 3:, 3:] = J[0], J[1], J[2]
        W = np.zeros((len(J[0]), 6, 6))
        for i in range(3):
            W[:, i, i], W[:, 3 + i, 3 + i] = wt, wr
        return np.einsum("mki,mkl,mlj->mij", Jf, W, Jf)

    Hc, Hl = blocks(P.cJ, P.wt, P.wr), blocks(P.lJ, P.lwt, P.lwr)
    He = np.zeros((te, 6, te, 6))
    for a, b, M in [(k, k + 1, Hc[k]) for k in range(te - 1)] + [(P.la[k], P.lb[k], Hl[k]) for k in range(len(P.la))]:
        He[b, :, b, :] += M
        He[a, :, a, :] += M
        He[a, :, b, :] -= M
        He[b, :, a, :] -= M
    S = np.kron(np.tril(np.ones((te, te))), np.eye(6))[:, 6:]                 # eta = S d with d_0 = 0 dropped
    D = np.zeros((6 * (te - 1), 6 * (te - 1)))
    for k in range(te - 1):
        D[6 * k:6 * k + 6, 6 * k:6 * k + 6] = Hc[k]
    return S.T @ He.reshape(6 * te, 6 * te) @ S, D


def test_preconditioned_matrix_is_identity_plus_rank_6L(scene):
    """The dense S^T H S of the first linearisation: its generalised eigenvalues against D are 1 except exactly 6 L of them; the
    restatement's product is that matrix; and with cg_iterations = 12 L its first step is the dense solve (1e-9 relative; measured
    3.9e-12 -- at 6 L + 1 iterations rounding leaves 5e-4, which is why that count is not tested)."""
    P = R.Problem(scene["odo"], scene["pairs"], scene["rel"], scene["weights"], *ODO)
    P.linearise()
    Hd, D = _dense_problem(P)
    nl = len(scene["pairs"])
    Lc = np.linalg.cholesky(D)
    M = np.linalg.solve(Lc, np.linalg.solve(Lc, Hd).T).T
    ev = np.linalg.eigvalsh((M + M.T) / 2)
    assert int((np.abs(ev - 1) > 1e-6).sum()) == 6 * nl and ev.min() > 1 - 1e-9
    rng = np.random.default_rng(0)
    p = np.zeros((P.te, 6))
    p[1:] = rng.normal(size=(P.te - 1, 6))
    hp = P.product(p)
    assert (hp[0] == 0).all() and np.abs(hp[1:].reshape(-1) - Hd @ p[1:].reshape(-1)).max() <= 1e-12 * np.abs(hp).max()
    dense = np.linalg.solve(Hd, -P.gradient()[1:].reshape(-1))
    x = P.solve(12 * nl)
    gap = np.abs(x[1:].reshape(-1) - dense).max() / np.abs(dense).max()
    print("CG with 12 L iterations against the dense solve: %.3e" % gap)
    assert (x[0] == 0).all() and gap <= 1e-9


def test_minimiser_agrees_with_scipy():
    """T = 24, 3 loops, iterations 6, cg_iterations 36: the poses against the minimiser scipy.optimize.least_squares (trf, every tolerance
    1e-15) finds for the same residual over the same retraction.  Measured gap: 4.5e-8 m in t and 1.3e-9 in R (scipy stops on its xtol;
    the restatement itself moves by 7e-15 between 6 and 12 iterations); the bounds are 10 times that and cover scipy's stopping only."""
    opt = pytest.importorskip("scipy.optimize")
    T = 24
    _, odo, pairs, rel, weights = R.circle_scene(T=T, loops=3)
    out = R.relax_reference(odo, pairs, rel, weights, *ODO, 6, 36)
    P = R.Problem(odo, pairs, rel, weights, *ODO)
    R0, c0 = P.R.copy(), P.c.copy()

    def moved(v):
        eta = np.zeros((T, 6))
        eta[1:] = v.reshape(T - 1, 6)
        return R.retract(R0, c0, eta)

    def resid(v):
        Rn, cn = moved(v)
        rt, rR, _ = R.residual(Rn[:-1], Rn[1:], cn[:-1], cn[1:], P.ZR, P.zt)
        lt, lR, _ = R.residual(Rn[P.la], Rn[P.lb], cn[P.la], cn[P.lb], P.lZR, P.lzt)
        return np.concatenate([(np.sqrt(P.wt)[:, None] * rt).ravel(), (np.sqrt(P.wr)[:, None] * rR).ravel(),
                               (np.sqrt(P.lwt)[:, None] * lt).ravel(), (np.sqrt(P.lwr)[:, None] * lR).ravel()])

    sol = opt.least_squares(resid, np.zeros(6 * (T - 1)), xtol=1e-15, ftol=1e-15, gtol=1e-15, method="trf")
    Rs, cs = moved(sol.x)
    m = out[0].reshape(T, 3, 4)
    gap_t, gap_R = np.abs(cs + P.t0 - m[:, :, 3]).max(), np.abs(Rs - m[:, :, :3]).max()
    print("against scipy: %.3e m, %.3e in R; cost %.6e / %.6e" % (gap_t, gap_R, 2 * sol.cost, out[1][-1]))
    assert gap_t <= 4.5e-7 and gap_R <= 1.3e-8
    assert abs(2 * sol.cost - out[1][-1]) <= 1e-12 * out[1][-1] + 1e-15


def test_cost_falls_and_the_trajectory_closes(scene):
    cost = scene["out"][1]
    print("cost:", cost.tolist())
    assert cost.shape == (5,) and (np.diff(cost) <= 0).all() and cost[-1] < 0.01 * cost[0]
    assert scene["out"][3].tolist() == [0, 0, 0] and scene["out"][4].tolist() == [64, 3]
    # the loops were exact: the relaxed trajectory is much nearer the truth than the odometry, and the loops' residuals are small
    assert np.abs(scene["out"][0] - scene["truth"]).max() < 0.2 * np.abs(scene["odo"] - scene["truth"]).max()
    assert (scene["out"][2] < 1e-3).all() and (scene["out"][2] >= 0).all()
    assert (scene["out"][0][0].view(np.int64) == scene["odo"][0].view(np.int64)).all()          # the anchor's bits


def test_gauge(scene):
    """Every input pose moved by one rigid motion with a UTM-sized translation moves every output by it: 1e-7 m, 1e-12 in R.  float64
    holds a UTM coordinate to 1e-9 m, so a scene that is moved THERE loses what the small one knew below that, and 1e-9 m over a 10 m
    edge turns the solution by more than 1e-12.  The test therefore starts from the scene in UTM coordinates and brings it back exactly
    (t - t_g is exact, then one rotation): both calls see the same trajectory."""
    for G in (R.pose_of([4.1e5, 5.5e6, 120.0], [0.1, -0.2, 2.0]), R.pose_of([-3.3e5, 6.1e6, 40.0], [0.0, 0.0, -1.0])):
        g = G.reshape(3, 4)
        far = np.stack([R.compose(G, o) for o in scene["odo"]])
        near = np.stack([np.concatenate([g[:, :3].T @ m[:, :3], g[:, :3].T @ (m[:, 3:] - g[:, 3:])], 1).reshape(12) for m in far.reshape(-1, 3, 4)])
        out_far = R.relax_reference(far, scene["pairs"], scene["rel"], scene["weights"], *ODO, 4, 36)
        out_near = R.relax_reference(near, scene["pairs"], scene["rel"], scene["weights"], *ODO, 4, 36)
        d = (out_far[0] - np.stack([R.compose(G, o) for o in out_near[0]])).reshape(-1, 3, 4)
        print("gauge: %.3e m, %.3e in R" % (np.abs(d[:, :, 3]).max(), np.abs(d[:, :, :3]).max()))
        assert np.abs(d[:, :, 3]).max() <= 1e-7 and np.abs(d[:, :, :3]).max() <= 1e-12
        assert np.abs(out_far[1] - out_near[1]).max() <= 1e-9 * out_near[1][0] and out_far[1][-1] < 0.01 * out_far[1][0]


def test_consistent_loops_move_nothing(scene):
    odo, pairs = scene["odo"], scene["pairs"]
    rel = np.stack([R.compose(R.inverse(odo[t]), odo[s]) for s, t in pairs])
    out = R.relax_reference(odo, pairs, rel, scene["weights"], *ODO, 4, 36)
    d = (out[0] - odo).reshape(-1, 3, 4)
    assert np.abs(d[:, :, 3]).max() <= 1e-9 and np.abs(d[:, :, :3]).max() <= 1e-12 and out[4].tolist() == [64, 3]
    assert (out[1] < 1e-20).all()


def test_rules(scene):
    odo, pairs, rel, weights = scene["odo"], scene["pairs"], scene["rel"], scene["weights"]
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    # no loop used: a bit copy and a zero cost -- with no loops at all, and with loops that are all skipped
    for p, r, w in ((np.zeros((0, 2), np.int32), np.zeros((0, 12)), np.zeros((0, 2))), (pairs, rel, np.zeros_like(weights))):
        out = R.relax_reference(odo, p, r, w, *ODO, 3, 5)
        assert (bits(out[0]) == bits(odo)).all() and (bits(out[1]) == 0).all() and out[1].shape == (4,)
        assert np.isnan(out[2]).all() and (out[3] == R.NO_EDGE).all() and out[4].tolist() == [64, 0]
    # a NaN pose at node 40: T_eff = 40, NaN rows behind it, every loop touching them flagged
    broken = odo.copy()
    broken[40, 2] = np.nan
    more = np.concatenate([pairs, [[10, 3], [39, 1], [40, 2], [5, 63]]]).astype(np.int32)
    mrel = np.concatenate([rel, [R.compose(R.inverse(odo[t]), odo[s]) for s, t in more[3:]]])
    mw = np.tile(np.array([[1.0, 100.0]]), (len(more), 1))
    out = R.relax_reference(broken, more, mrel, mw, *ODO, 2, 12)
    assert out[4].tolist() == [40, 3] and np.isnan(out[0][40:]).all() and np.isfinite(out[0][:40]).all()
    assert out[3].tolist() == [R.NO_EDGE if max(s, t) >= 40 else 0 for s, t in more] and out[3].tolist().count(0) == 3 and out[3][0] == 0
    assert np.isnan(out[2][out[3] != 0]).all() and np.isfinite(out[2][out[3] == 0]).all()
    # each skip reason alone, beside one good loop
    good = (more[3], mrel[3], mw[3])
    reasons = {"source outside": dict(pair=(-1, 3)), "target outside": dict(pair=(3, 64)), "source == target": dict(pair=(7, 7)),
               "rel NaN": dict(rel=5, value=np.nan), "rel Inf": dict(rel=11, value=-np.inf), "weight NaN": dict(w=(np.nan, 1.0)),
               "weight Inf": dict(w=(1.0, np.inf)), "weight negative": dict(w=(-1e-300, 1.0)), "both weights 0": dict(w=(0.0, 0.0))}
    for name, kw in reasons.items():
        p2 = np.array([good[0], kw.get("pair", (20, 4))], np.int32)
        r2 = np.stack([good[1], R.compose(R.inverse(odo[4]), odo[20])])
        w2 = np.array([good[2], kw.get("w", (1.0, 100.0))])
        if "rel" in kw:
            r2[1, kw["rel"]] = kw["value"]
        out = R.relax_reference(odo, p2, r2, w2, *ODO, 1, 6)
        assert out[3].tolist() == [0, R.NO_EDGE] and out[4].tolist() == [64, 1] and np.isnan(out[2][1]) and np.isfinite(out[2][0]), name
    for w in ((0.0, 1.0), (1.0, 0.0), (-0.0, 3.0)):                           # one zero weight alone is a used loop
        out = R.relax_reference(odo, good[0][None], good[1][None], np.array([w]), *ODO, 1, 6)
        assert out[3].tolist() == [0] and out[4].tolist() == [64, 1], w
    # a pivot that is not > 0 (odometry weights under which D overflows: Inf / Inf is the next pivot): the input comes back and
    # num_out[1] says so
    out = R.relax_reference(odo, pairs, rel, weights, 1e308, 1e308, 1, 3)
    assert out[4].tolist() == [64, -1] and (bits(out[0]) == bits(odo)).all() and (bits(out[1]) == 0).all() and np.isnan(out[2]).all()
