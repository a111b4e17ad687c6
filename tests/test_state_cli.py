"""State API, CLI, and job submission tests."""
import os
import time

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ray_mod():
    import ant_ray_amd as ray

    if ray.is_initialized():
        ray.shutdown()  # never inherit another module's (possibly dying) session
    if not ray.is_initialized():
        ray.init(num_cpus=8)
    yield ray
    ray.shutdown()


def test_state_lists(ray_mod):
    ray = ray_mod
    from ant_ray_amd.util import state

    @ray.remote
    def noop(i):
        return i

    @ray.remote
    class Named:
        def ping(self):
            return "pong"

    a = Named.options(name="state_test_actor").remote()
    assert ray.get(a.ping.remote()) == "pong"
    ray.get([noop.remote(i) for i in range(20)])

    actors = state.list_actors()
    assert any(x["name"] == "state_test_actor" for x in actors)
    nodes = state.list_nodes()
    assert len(nodes) >= 1
    # task events are flushed in batches (<=1s cadence)
    deadline = time.time() + 10
    tasks = []
    while time.time() < deadline:
        tasks = state.list_tasks(limit=5000)
        if sum(1 for t in tasks if t.get("name") == "noop") >= 20:
            break
        time.sleep(0.3)
    assert sum(1 for t in tasks if t.get("name") == "noop") >= 20
    assert all(t["state"] in ("FINISHED", "FAILED") for t in tasks)

    trace = state.get_timeline()
    assert len(trace) >= 20
    ev = next(e for e in trace if e["name"] == "noop")
    assert ev["ph"] == "X" and ev["dur"] >= 1


def test_cli_status_and_list(ray_mod):
    from click.testing import CliRunner

    from ant_ray_amd.scripts.cli import cli

    r = CliRunner().invoke(cli, ["status"])
    assert r.exit_code == 0, r.output
    assert "Nodes: " in r.output
    r = CliRunner().invoke(cli, ["list", "actors"])
    assert r.exit_code == 0, r.output
    assert "state_test_actor" in r.output


def test_cli_timeline(ray_mod, tmp_path):
    from click.testing import CliRunner

    from ant_ray_amd.scripts.cli import cli

    out = str(tmp_path / "trace.json")
    r = CliRunner().invoke(cli, ["timeline", "-o", out])
    assert r.exit_code == 0, r.output
    import json

    trace = json.load(open(out))
    assert isinstance(trace, list) and trace


def test_job_submission(ray_mod):
    from ant_ray_amd.job_submission import JobSubmissionClient

    client = JobSubmissionClient()
    job_id = client.submit_job(
        entrypoint="python -c \"print('hello from job 12321')\"")
    deadline = time.time() + 60
    while time.time() < deadline:
        st = client.get_job_status(job_id)
        if st in ("SUCCEEDED", "FAILED"):
            break
        time.sleep(0.5)
    assert st == "SUCCEEDED"
    assert "hello from job 12321" in client.get_job_logs(job_id)
    jobs = client.list_jobs()
    assert any(j["submission_id"] == job_id for j in jobs)


def test_cli_memory(ray_mod):
    """`ray memory` prints per-node object-store usage from the raylet's
    shm stats (parity: reference ray memory / raylet GetNodeStats)."""
    import numpy as np

    from click.testing import CliRunner

    from ant_ray_amd.scripts.cli import cli
    from ant_ray_amd.util import state

    ray = ray_mod
    keep = ray.put(np.zeros(1 << 20, dtype=np.uint8))  # 1 MiB in shm

    rows = state.store_stats()
    assert rows, "expected at least the head node's store stats"
    assert rows[0]["arena_size"] > 0
    assert any(r["total_created"] >= 1 for r in rows)

    r = CliRunner().invoke(cli, ["memory"])
    assert r.exit_code == 0, r.output
    assert "MiB used" in r.output
    del keep


def test_logs_and_summaries(ray_mod):
    from click.testing import CliRunner

    from ant_ray_amd.scripts.cli import cli
    from ant_ray_amd.util import state

    logs = state.list_logs()
    assert isinstance(logs, list)
    if logs:
        assert isinstance(state.get_log(logs[0], tail=10), str)
    assert isinstance(state.summarize_actors(), list)
    r = CliRunner().invoke(cli, ["summary", "actors"])
    assert r.exit_code == 0, r.output


def test_llm_alias_imports():
    import ant_ray_amd.data.llm as dllm
    import ant_ray_amd.serve.llm as sllm

    assert hasattr(sllm, "build_openai_app")
    assert hasattr(dllm, "build_llm_processor")


def test_cli_logs_health_stack_drain(ray_mod):
    """New CLI commands: logs / health-check / stack / drain-node
    (parity: reference scripts/scripts.py surface)."""
    import subprocess
    import sys

    env = dict(os.environ)
    env["PYTHONPATH"] = REPO

    def run(*args):
        return subprocess.run(
            [sys.executable, "-m", "ant_ray_amd.scripts.cli", *args],
            capture_output=True, text=True, env=env, timeout=120)

    r = run("health-check")
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)

    r = run("logs")
    assert r.returncode == 0, r.stderr

    r = run("stack")
    assert r.returncode == 0, r.stderr
    assert "signaled" in r.stdout or "no runtime processes" in r.stdout

    r = run("disable-usage-stats")
    assert r.returncode == 0 and "disabled" in r.stdout


def test_state_getters_and_client(ray_mod):
    """get_task/get_worker/get_job/get_objects/list_runtime_envs +
    StateApiClient (parity: util/state/api.py)."""
    import ant_ray_amd as ray
    from ant_ray_amd.util import state as S
    from ant_ray_amd.util.state import StateApiClient

    @ray.remote
    def probe():
        return 1

    ray.get([probe.remote() for _ in range(3)], timeout=60)
    tasks = S.list_tasks(limit=100)
    assert tasks
    tid = tasks[0].get("task_id")
    if isinstance(tid, bytes):
        tid = tid.hex()
    assert S.get_task(tid) is not None

    workers = S.list_workers(limit=10)
    if workers:
        assert S.get_worker(workers[0]["worker_id"]) is not None

    c = StateApiClient()
    assert isinstance(c.list("actors"), list)
    assert isinstance(c.list("nodes"), list)
    assert isinstance(c.list("runtime_envs"), list)
    with pytest.raises(ValueError):
        c.list("nope")
    nodes = c.list("nodes")
    assert c.get("nodes", nodes[0]["node_id"]) is not None
