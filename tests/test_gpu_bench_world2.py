"""bench.py's N > 1 code path, run once before the driver's 8-GPU run does: `bench.py --full --gpus 2 --backend
gloo --same-device` -- the script launches itself under torch.distributed.run, both ranks on cuda:0 (RCCL refuses two ranks on one GPU, so
the dry run's backend is gloo) -- must print ONE JSON line from rank 0, report the backend truthfully, run every `configs` leg on both
ranks without an error, and its sharded retrieval must book exactly what the one-rank run books (integer counters: SURVEY.md 8e).
bench.py starts as a CHILD of the test process.  Numbers from this run are not credit.
A plain run (no --full) is checked as well: the headline alone, exactly --steps timed steps, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, full=True):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--settle-ms", "0"]
    if full:
        cmd += ["--full", "--regions", "1", "--no-cpu-baseline", "--precision", "f32", "--in-flight", "1"]
    cmd += list(flags)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert p.returncode == 0, "bench.py %s exited %d:\n%s" % (" ".join(flags), p.returncode, p.stderr.decode()[-3000:])
    assert len(lines) == 1, "expected ONE line on stdout, got %d:\n%s" % (len(lines), "\n".join(ln[:200] for ln in lines))
    return json.loads(lines[0])


def test_bench_runs_its_two_rank_code_on_one_device():
    two = _bench("--gpus", "2", "--backend", "gloo", "--same-device")
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["steps"] == 3
    assert two["backend"] == {"name": "gloo", "rccl": False, "ranks": 2, "same_device": True}
    legs = two["configs"]
    assert set(legs) >= {"train_step", "train_step_bf16", "train_step_22", "train_step_bf16_22", "epc_net_l_b256", "retrieval"}
    for name, leg in legs.items():
        assert "error" not in leg, (name, leg)
    r2 = legs["retrieval"]
    assert r2["rccl_exercised"] is False and r2["rccl_ranks"] == 0 and r2["ranks"] == 2 and r2["backend"] == "gloo"
    assert "three graphs" in legs["train_step"]["workload"] and legs["train_step_22"]["clouds_per_tuple"] == 22
    # the one-rank run of the same script: the sharded evaluation's results do not depend on the sharding
    one = _bench("--gpus", "1", "--backend", "gloo")
    r1 = one["configs"]["retrieval"]
    assert one["backend"]["ranks"] == 1 and r1["ranks"] == 1
    for key in ("ave_recall_at_1", "ave_one_percent_recall", "average_similarity", "queries_ranked", "ordered_pairs"):
        assert r1[key] == r2[key], (key, r1[key], r2[key])
    # (no assertion on the rates: three-step regions on a box that has just run another GPU process are dominated by one dispatch
    # stall -- 2 k clouds/s was seen for a run that does 58 k -- and numbers from a dry run are not credit anyway)
    assert two["value"] > 0 and one["value"] > 0


def test_plain_run_times_the_headline_alone_and_dumps_its_descriptors(tmp_path):
    """No --full: one region of exactly --steps steps, none of the --full objects on the line, and --dump-outputs writes the
    descriptors of the last timed step -- unit-norm, and the same on a second run with the same arguments (seeded inputs)."""
    dumps = [str(tmp_path / d) for d in ("a", "b")]
    for d in dumps:
        line = _bench("--gpus", "1", "--dump-outputs", d, full=False)
        assert line["full"] is False and line["steps"] == 3 and line["regions"]["count"] == 1 and line["regions"]["steps_each"] == 3
        assert not set(line) & {"roofline", "stage_ms", "overlapped", "fast", "configs", "pipeline_hbm", "cpu_baseline"}, sorted(line)
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f16x3" and line["backend"]["rccl"] is False
    a, b = (np.load(os.path.join(d, "descriptors.npy")) for d in dumps)
    assert a.shape == (64, 256) and a.dtype == np.float32
    assert float(np.abs(np.linalg.norm(a, axis=1) - 1.0).max()) <= 1e-3
    assert np.array_equal(a, b)
