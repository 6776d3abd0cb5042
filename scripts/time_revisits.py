"""The revisit search against the square search it replaces, and one streaming add, at T = 4096 and 32 768 submaps (dim 256, k 5, along =
arange(T) * 10, min_travel 100): per T (a) the median time of retrieval.revisit_search on the trajectory against itself, (b) the median
time of retrieval.knn_search(desc, desc, 5) on the same rows -- the full square, measured in the same process, the arms alternating --
and (c) the time of one RevisitIndex.add of a single row at that fill level.  HIP events around `--steps` calls, `--regions` regions, the
median region; everything runs eagerly on one stream.  The expectation to report against: the triangular search is not slower than the
square one (about half the GEMM and half the selection's scans, plus the prepare launches); the JSON says which way it came out.

Without --one the script touches no device itself: it starts one child process per T (`--one T`) under a time limit of its own, stops at
the first child that fails, and writes the children's lines as one JSON document, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_revisits.py [--sizes 4096,32768] [--steps K] [--regions R] [--warmup W] [--limit SECONDS] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _timing  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r13_revisit_time.json")

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,32768")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--min-travel", type=float, default=100.0)
ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
ap.add_argument("--one", type=int, default=0, help="(child) measure this T and print its JSON line")
ap.add_argument("--out", default=DEFAULT_OUT)
args = ap.parse_args()

if not args.one:
    lines = _timing.children(__file__, args.sizes.split(","), ["--steps", args.steps, "--regions", args.regions, "--warmup", args.warmup,
                                                                "--dim", args.dim, "--k", args.k, "--min-travel", args.min_travel], args.limit)
    _timing.emit({"workload": "one trajectory of T submaps searched against itself: dim %d, k %d, along = arange(T) * 10, min_travel %g"
                              % (args.dim, args.k, args.min_travel),
                  "timer": "HIP events around %d calls; median of %d regions, the arms alternating; eager, one stream; one process per T"
                           % (args.steps, args.regions),
                  "expectation": "revisit_search is not slower than knn_search(desc, desc, k) on the same rows",
                  "sizes": lines, "lib_sha256": lines[0]["lib_sha256"]}, args.out)
    raise SystemExit(0)

import torch  # noqa: E402

import bench  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_revisits.py measures on the device: no ROCm device is visible")
RT, L = bench.pkg("retrieval"), bench.pkg("lib")
dev = torch.device("cuda:0")
T, dim, k = args.one, args.dim, args.k
gen = torch.Generator(device="cpu").manual_seed(T)
desc = torch.randn((T, dim), generator=gen, dtype=torch.float32)
desc = (desc / desc.norm(dim=1, keepdim=True)).to(dev)
along = (torch.arange(T, dtype=torch.float64) * 10.0).to(dev)
ws = torch.empty(int(L.lib().epcnet_revisit_workspace_bytes(T, T, 0)), dtype=torch.uint8, device=dev)

# the timed calls compute what they should: the counts, and the last row against the square search on its prefix
dist, idx, count = RT.revisit_search(desc, along, args.min_travel, k, workspace=ws)
torch.cuda.synchronize()
want_count = torch.clamp(torch.arange(T) - int(args.min_travel / 10.0) + 1, min=0).to(torch.int32)
assert torch.equal(count.cpu(), want_count), "count"
p = int(count[-1])
d_ref, i_ref = RT.knn_search(desc[:p], desc[-1:], k)
assert torch.equal(i_ref, idx[-1:]) and torch.equal(d_ref.view(torch.int32), dist[-1:].view(torch.int32)), "the last row is the square search's"

index = RT.RevisitIndex(T, dim=dim, min_travel=args.min_travel, k=k, device=dev)
index.add(desc[:T - 1], along[:T - 1])
last_desc, last_along = desc[T - 1:].clone(), along[T - 1:].clone()


def add_one():
    index.truncate(T - 1)
    return index.add(last_desc, last_along)


got = add_one()
torch.cuda.synchronize()
assert torch.equal(got[1], idx[-1:]) and torch.equal(got[2], count[-1:]), "the streamed row is the batch call's"

arms = {"revisit_search": lambda: RT.revisit_search(desc, along, args.min_travel, k, workspace=ws),
        "knn_search_square": lambda: RT.knn_search(desc, desc, k),
        "index_add_one_row": add_one}
times = {name: [1e3 * t / args.steps for t in v]                             # seconds per region -> ms per call
         for name, v in _timing.alternate(arms, args.steps, args.regions, args.warmup, events=True).items()}
ms = {name: statistics.median(v) for name, v in times.items()}
ratio = ms["revisit_search"] / ms["knn_search_square"]
_timing.emit({"T": T, "ms_per_call": {n: round(v, 4) for n, v in ms.items()},
              "regions_ms": {n: [round(t, 4) for t in v] for n, v in times.items()},
              "revisit_over_square": round(ratio, 3),
              "verdict": "not slower than the square search" if ratio <= 1.0 else "SLOWER than the square search"})
