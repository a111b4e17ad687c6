"""The driver's bench contract, CPU plumbing: torchrun spawns N ranks;
in via-ray mode rank 0 alone drives ray + TorchTrainer (worker actors are
the ranks) and prints ONE JSON line; sibling ranks exit 0 untouched.
ANTRAY_BENCH_CPU=1 runs the identical launch shape on CPU/gloo with the
tiny model so this exact path is covered before the driver's first
8-GPU scaling run."""
import json
import os
import subprocess
import sys


def test_via_ray_torchrun_cpu_2ranks(tmp_path):
    env = dict(os.environ, ANTRAY_BENCH_CPU="1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29721", "bench.py", "--gpus", "2",
         "--model", "llama-tiny", "--seq", "64", "--batch", "2",
         "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=600, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # exactly ONE JSON line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["via"] == "ray-train"
    assert rec["value"] > 0
    # --dump-outputs: the last timed step's loss + updated optimizer state
    import numpy as np

    dumped = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(dumped) == {"loss", "params", "exp_avg", "exp_avg_sq"}
    assert all(a.dtype in (np.float32, np.float64) for a in dumped.values())
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20
    assert abs(float(dumped["loss"][0]) - rec["config"]["final_loss"]) < 1e-3


def test_bare_mode_flag():
    import bench

    a = bench._parse_args(["--bare", "--steps", "4"])
    assert a.bare and a.steps == 4
