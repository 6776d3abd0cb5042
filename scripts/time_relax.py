"""Trajectory relaxation against the same iteration written with torch, at (T, L) = (4096, 64) and (32768, 1024) and one streaming-sized
call of (4096, 5), iterations 4 and cg_iterations 64: per size (a) the median time of one retrieval.relax_trajectory call, eager and as a
replayed graph, (b) in the same process the same Gauss-Newton / preconditioned-CG iteration in chain-increment variables done the way a
user would do it without these kernels -- float64 torch on the device: cumsum for the scans, index_add_ for the loops' scatter, batched
matmul for the 6 x 6 work and the preconditioner (the blocks' inverses, formed once per linearisation), nothing read back -- and (c)
both at half the CG iterations, so that the time of ONE CG iteration is the difference and not a share of the fixed work.  HIP events around `--steps` calls, `--regions` regions, the
median region, the arms alternating; one stream.  The bar set in advance: the eager call is not slower than the torch arm at any size;
the JSON says which way it came out.

Without --one the script touches no device itself: it starts one child process per size (`--one T,L`) under a time limit of its own,
stops at the first child that fails, and writes the children's lines as one JSON document, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_relax.py [--sizes 4096x64,32768x1024,4096x5] [--steps K] [--regions R] [--warmup W] [--limit SECONDS]
[--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _timing  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r15_relax_time.json")

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096x64,32768x1024,4096x5")
ap.add_argument("--iterations", type=int, default=4)
ap.add_argument("--cg", type=int, default=64)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--regions", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
ap.add_argument("--one", default="", help="(child) measure this T,L and print its JSON line")
ap.add_argument("--out", default=DEFAULT_OUT)
args = ap.parse_args()

if not args.one:
    lines = _timing.children(__file__, [size.replace("x", ",") for size in args.sizes.split(",")],
                             ["--steps", args.steps, "--regions", args.regions, "--warmup", args.warmup, "--iterations", args.iterations,
                              "--cg", args.cg], args.limit)
    slower = [(l["T"], l["L"]) for l in lines if l["entry_over_torch"] > 1.0]
    _timing.emit({"workload": "a wandering trajectory of T submaps, 5 m apart, with L loops between random nodes; iterations %d, cg_iterations %d, "
                              "odometry weights (1, 100)" % (args.iterations, args.cg),
                  "timer": "HIP events around %d calls; median of %d regions, the arms alternating; one stream; one process per size"
                           % (args.steps, args.regions),
                  "bar": "the eager call is not slower than the same iteration written with torch (cumsum, index_add_, batched matmul) on the device",
                  "verdict": "met at every size" if not slower else "MISSED at (T, L) = %s" % slower,
                  "not_measured": "no kernel trace was taken: the shares of launch latency, scans and edge work inside a CG iteration are not known",
                  "sizes": lines, "lib_sha256": lines[0]["lib_sha256"]}, args.out)
    raise SystemExit(0)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import relax_ref as R  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_relax.py measures on the device: no ROCm device is visible")
RT, L = bench.pkg("retrieval"), bench.pkg("lib")
dev = torch.device("cuda:0")
T, nl = (int(v) for v in args.one.split(","))
odo_h, pairs_h, rel_h, weights_h = R.walk_scene(T, nl, seed=15, noise_t=0.02, noise_r=0.0005)
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
odo, pairs, rel, weights = up(odo_h, np.float64), up(pairs_h, np.int32), up(rel_h, np.float64), up(weights_h, np.float64)
ws = torch.empty(int(L.lib().epcnet_trajectory_relax_workspace_bytes(T, nl)), dtype=torch.uint8, device=dev)
WT, WR = 1.0, 100.0

# the timed calls compute what they should: a short prefix against the restatement, bit for bit
few_T, few_L = 600, min(nl, 5)
keep = [e for e in range(nl) if max(pairs_h[e]) < few_T][:few_L]
got = RT.relax_trajectory(odo[:few_T].contiguous(), pairs[keep].contiguous(), rel[keep].contiguous(), weights[keep].contiguous(), (WT, WR), 2, 8)
torch.cuda.synchronize()
want = R.relax_reference(odo_h[:few_T], pairs_h[keep], rel_h[keep], weights_h[keep], WT, WR, 2, 8)
assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().tobytes() == want[1].tobytes(), "the entry equals its restatement"

src, tgt = pairs[:, 0].long(), pairs[:, 1].long()
EYE = torch.eye(3, dtype=torch.float64, device=dev)
EYE6 = torch.eye(6, dtype=torch.float64, device=dev)


def skew(v):
    o = torch.zeros_like(v[:, 0])
    return torch.stack([o, -v[:, 2], v[:, 1], v[:, 2], o, -v[:, 0], -v[:, 1], v[:, 0], o], 1).reshape(-1, 3, 3)


def torch_relax(iterations, cg):
    """The same iteration in float64 torch; every loop is taken as used (the scene has no skipped one); no host read."""
    m = odo.reshape(T, 3, 4)
    Rn, c = m[:, :, :3].clone(), m[:, :, 3] - m[0, :, 3]
    a = torch.cat([torch.arange(T - 1, device=dev), tgt])
    b = torch.cat([torch.arange(1, T, device=dev), src])
    rm = rel.reshape(nl, 3, 4)
    ZR = torch.cat([Rn[:-1].transpose(1, 2) @ Rn[1:], rm[:, :, :3]])
    zt = torch.cat([(Rn[:-1].transpose(1, 2) @ (c[1:] - c[:-1]).unsqueeze(2)).squeeze(2), rm[:, :, 3]])
    w = torch.cat([torch.tensor([[WT, WT, WT, WR, WR, WR]], dtype=torch.float64, device=dev).expand(T - 1, 6),
                   weights[:, [0, 0, 0, 1, 1, 1]]])
    costs = []

    def linearise():
        A = Rn[a].transpose(1, 2)
        cb = c[b]
        rt = (A @ (cb - c[a]).unsqueeze(2)).squeeze(2) - zt
        E = ZR.transpose(1, 2) @ (A @ Rn[b])
        rR = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
        tr = E.diagonal(dim1=1, dim2=2).sum(1)
        C = 0.5 * (tr.reshape(-1, 1, 1) * EYE - E.transpose(1, 2)) @ Rn[b].transpose(1, 2)
        J = torch.zeros((T - 1 + nl, 6, 6), dtype=torch.float64, device=dev)
        J[:, :3, :3], J[:, :3, 3:], J[:, 3:, 3:] = A, -(A @ skew(cb)), C
        r = torch.cat([rt, rR], 1)
        JW = J.transpose(1, 2) * w.unsqueeze(1)
        return JW @ J, (JW @ r.unsqueeze(2)).squeeze(2), (w * r * r).sum()

    def assemble(v, u):
        g = torch.zeros((T + 1, 6), dtype=torch.float64, device=dev)
        g.index_add_(0, tgt + 1, u)
        g.index_add_(0, src + 1, -u)
        out = torch.zeros((T, 6), dtype=torch.float64, device=dev)
        out[1:] = v + torch.cumsum(g[:T], 0)[1:]
        return out

    def block_inverse(D):
        """D^-1 of the (T - 1, 6, 6) blocks from a Cholesky factor and its inverse, a column / a row at a time with elementwise torch and
        matmul: on the ROCm build this was written on, torch.cholesky_solve returned a z with |D z - r| 1e17 times the CPU's from its
        third call on (the same D, r equal to 2e-12), and the CG of this arm diverged; nothing of the LAPACK family is used here."""
        Lc = torch.zeros_like(D)
        for j in range(6):
            col = D[:, j:, j] - (Lc[:, j:, :j] @ Lc[:, j, :j].unsqueeze(2)).squeeze(2)
            Lc[:, j:, j] = col / torch.sqrt(col[:, :1])
        Li = torch.zeros_like(D)
        for i in range(6):
            Li[:, i, :] = (EYE6[i] - (Lc[:, i:i + 1, :i] @ Li[:, :i, :]).squeeze(1)) / Lc[:, i, i:i + 1]
        return Li.transpose(1, 2) @ Li

    for _ in range(iterations):
        Hb, gb, cost = linearise()
        costs.append(cost)
        Dinv = block_inverse(Hb[:T - 1])

        def precondition(r):
            z = torch.zeros_like(r)
            z[1:] = (Dinv @ r[1:].unsqueeze(2)).squeeze(2)
            return z

        def product(p):
            eta = torch.cumsum(p, 0)
            return assemble((Hb[:T - 1] @ p[1:].unsqueeze(2)).squeeze(2), (Hb[T - 1:] @ (eta[src] - eta[tgt]).unsqueeze(2)).squeeze(2))

        r = -assemble(gb[:T - 1], gb[T - 1:])
        x = torch.zeros_like(r)
        z = precondition(r)
        p = z.clone()
        rz = (r * z).sum()
        for _ in range(cg):
            hp = product(p)
            alpha = rz / (p * hp).sum()
            x = x + alpha * p
            r = r - alpha * hp
            z = precondition(r)
            rz_new = (r * z).sum()
            p = z + (rz_new / rz) * p
            rz = rz_new
        eta = torch.cumsum(x, 0)
        q = 0.5 * eta[:, 3:]
        u = 2.0 / (1.0 + (q * q).sum(1))
        K = skew(q)
        Cw = EYE + u.reshape(-1, 1, 1) * (K + K @ K)
        Rn, c = Cw @ Rn, (Cw @ c.unsqueeze(2)).squeeze(2) + eta[:, :3]
    costs.append(linearise()[2])
    return Rn, c, torch.stack(costs)


# the torch arm does the same work: its costs after one short solve against the entry's (1e-7 apart on the CPU: another preconditioner
# arithmetic, and CG at these sizes carries rounding forward; after a few hundred CG iterations the two no longer agree at all)
entry_cost = RT.relax_trajectory(odo, pairs, rel, weights, (WT, WR), 1, 8, workspace=ws)[1].cpu().numpy()
torch_cost = torch_relax(1, 8)[2].cpu().numpy()
assert np.allclose(entry_cost, torch_cost, rtol=1e-4, atol=0), (entry_cost, torch_cost)

half = max(args.cg // 2, 1)
graphs = {}
for name, cg in (("entry_graph", args.cg),):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        RT.relax_trajectory(odo, pairs, rel, weights, (WT, WR), args.iterations, cg, workspace=ws)
    torch.cuda.current_stream().wait_stream(stream)
    graphs[name] = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs[name]):
        held = RT.relax_trajectory(odo, pairs, rel, weights, (WT, WR), args.iterations, cg, workspace=ws)

arms = {"entry": lambda: RT.relax_trajectory(odo, pairs, rel, weights, (WT, WR), args.iterations, args.cg, workspace=ws),
        "torch": lambda: torch_relax(args.iterations, args.cg),
        "entry_half_cg": lambda: RT.relax_trajectory(odo, pairs, rel, weights, (WT, WR), args.iterations, half, workspace=ws),
        "torch_half_cg": lambda: torch_relax(args.iterations, half),
        "entry_graph": graphs["entry_graph"].replay}
times = {name: [1e3 * t / args.steps for t in v]                             # seconds per region -> ms per call
         for name, v in _timing.alternate(arms, args.steps, args.regions, args.warmup, events=True).items()}
ms = {name: statistics.median(v) for name, v in times.items()}
ratio = ms["entry"] / ms["torch"]
per_cg = lambda full, part: (ms[full] - ms[part]) / (args.iterations * (args.cg - half)) if args.cg > half else None
launches = 4 + args.iterations * (7 + 7 * args.cg) + 4
_timing.emit({"T": T, "L": nl, "iterations": args.iterations, "cg_iterations": args.cg, "launches_per_call": launches,
              "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
              "regions_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
              "us_per_cg_iteration": {"entry": round(1e3 * per_cg("entry", "entry_half_cg"), 2),
                                      "torch": round(1e3 * per_cg("torch", "torch_half_cg"), 2)},
              "us_per_launch_in_graph": round(1e3 * ms["entry_graph"] / launches, 3),
              "entry_over_torch": round(ratio, 3),
              "verdict": "not slower than the torch arm" if ratio <= 1.0 else "SLOWER than the torch arm"})
