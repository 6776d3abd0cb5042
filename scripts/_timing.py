"""What the timing scripts of the scan front end and of loop closing share (time_downsample.py, time_ground.py, time_submap.py,
time_deskew.py; time_revisits.py, time_register.py, time_relax.py): the compiler's resource remarks per kernel, one child process per
case, the loop of alternating arms, and the JSON line stamped with the SHA-256 of the loaded library."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epc-net_amd", "csrc")
# the Makefile's flags (csrc/Makefile: CXXFLAGS, without the warnings)
HIPCC_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize"]


def kernel_resources(source, name_regex):
    """{kernel: registers, LDS, scratch, spills, occupancy} of the kernels of ``source`` (a file of csrc, or any path) whose name matches
    ``name_regex``, from hipcc's resource remarks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out = {}
    for block in text.split("Function Name:")[1:]:
        name = re.search(name_regex, block.split("\n", 1)[0])
        if not name:
            continue
        grab = lambda key: int(re.search(r"\b%s:\s*(\d+)" % re.escape(key), block).group(1))
        out[name.group(0)] = {"vgprs": grab("VGPRs"), "sgprs": grab("TotalSGPRs"), "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
                              "vgpr_spills": grab("VGPRs Spill"), "lds_bytes": grab("LDS Size [bytes/block]"),
                              "waves_per_simd": grab("Occupancy [waves/SIMD]")}
    return out


def children(script, cases, passed_on, limit):
    """The parent half of a script that measures one case per process and touches no device itself: ``script --one <case>`` with the
    arguments ``passed_on``, one child at a time, each under ``limit`` seconds -> the last stdout line of every child, parsed as JSON
    (and printed as it arrives).  The first child that exits non-zero or runs out of time ends the run: nothing further is started."""
    lines = []
    for case in cases:
        cmd = [sys.executable, os.path.abspath(script), "--one", case] + [str(a) for a in passed_on]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a child past its limit is killed
        except subprocess.TimeoutExpired:
            raise SystemExit("--one %s did not end within %d s; nothing further is started" % (case, limit))
        if r.returncode != 0:
            raise SystemExit("--one %s failed (%d); nothing further is started\n%s" % (case, r.returncode, r.stderr[-2000:]))
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def alternate(arms, steps, regions, warmup, events=False):
    """``warmup`` calls of every arm, then ``regions`` rounds over the arms, each arm's region ``steps`` calls between device
    synchronisations -> {arm: [seconds per region]}.  The clock is the host's, or, ``events``, a pair of HIP events around the calls."""
    import torch
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(regions):
        for k, fn in arms.items():
            if events:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            if events:
                start.record()
            else:
                t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            if events:
                end.record()
                end.synchronize()
                times[k].append(start.elapsed_time(end) * 1e-3)
            else:
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    return times


def emit(line, out=None):
    """Stamp ``line`` with the loaded library's SHA-256 (a parent of ``children`` loads none: its line carries a child's stamp already),
    print it as one JSON line and, ``out``, write it to that file too."""
    if "lib_sha256" not in line:
        import bench
        line["lib_sha256"] = bench.lib_sha256()
    text = json.dumps(line)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
