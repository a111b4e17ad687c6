"""Tests: ray.util.queue / ActorPool / metrics, and the dashboard REST head."""
import json
import os
import time
import urllib.request

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


def test_queue(ray_mod):
    from ant_ray_amd.util.queue import Empty, Queue

    q = Queue(maxsize=3)
    q.put(1)
    q.put(2)
    assert q.qsize() == 2
    assert q.get() == 1
    assert q.get(timeout=5) == 2
    with pytest.raises(Empty):
        q.get(block=False)
    q.shutdown()


def test_queue_producer_consumer(ray_mod):
    ray = ray_mod
    from ant_ray_amd.util.queue import Queue

    q = Queue()

    @ray.remote
    def producer(q, n):
        for i in range(n):
            q.put(i)
        return n

    @ray.remote
    def consumer(q, n):
        return sum(q.get(timeout=30) for _ in range(n))

    p = producer.remote(q, 10)
    c = consumer.remote(q, 10)
    assert ray.get(c, timeout=60) == 45
    assert ray.get(p) == 10
    q.shutdown()


def test_actor_pool(ray_mod):
    ray = ray_mod
    from ant_ray_amd.util.actor_pool import ActorPool

    @ray.remote
    class Sq:
        def sq(self, x):
            return x * x

    pool = ActorPool([Sq.remote() for _ in range(3)])
    out = list(pool.map(lambda a, v: a.sq.remote(v), range(10)))
    assert out == [i * i for i in range(10)]
    out = sorted(pool.map_unordered(lambda a, v: a.sq.remote(v), range(6)))
    assert out == [i * i for i in range(6)]


def test_metrics_and_dashboard(ray_mod):
    import ant_ray_amd as ray
    from ant_ray_amd.dashboard import start_dashboard
    from ant_ray_amd.util.metrics import Counter, Gauge, Histogram

    c = Counter("test_requests_total", tag_keys=("route",))
    c.inc(1, {"route": "/a"})
    c.inc(2, {"route": "/a"})
    g = Gauge("test_temp", tag_keys=())
    g.set(42.5)
    h = Histogram("test_lat", boundaries=[0.1, 1.0], tag_keys=())
    h.observe(0.05)
    h.observe(0.5)
    h.observe(5.0)

    port = start_dashboard(port=0 or 8277)
    base = f"http://127.0.0.1:{port}"

    with urllib.request.urlopen(f"{base}/healthz", timeout=10) as r:
        assert r.read() == b"ok"
    with urllib.request.urlopen(f"{base}/api/cluster_status", timeout=10) as r:
        st = json.loads(r.read())
    assert st["nodes"] and "resources" in st
    with urllib.request.urlopen(f"{base}/api/actors", timeout=10) as r:
        assert isinstance(json.loads(r.read()), list)
    with urllib.request.urlopen(f"{base}/api/memory", timeout=10) as r:
        mem = json.loads(r.read())
    assert mem and "arena_size" in mem[0]
    with urllib.request.urlopen(f"{base}/api/cluster_events", timeout=10) as r:
        assert isinstance(json.loads(r.read()), list)
    with urllib.request.urlopen(f"{base}/api/logs", timeout=10) as r:
        logs = json.loads(r.read())
    assert isinstance(logs, list)
    # per-node reporter (dashboard/reporter.py in each raylet, 5s period):
    # wait for the first sample and check the psutil-backed fields
    deadline = time.time() + 30
    stats = {}
    while time.time() < deadline and not stats:
        with urllib.request.urlopen(f"{base}/api/node_stats",
                                    timeout=10) as r:
            stats = json.loads(r.read())
        if not stats:
            time.sleep(1)
    assert stats, "no reporter samples arrived"
    rec = next(iter(stats.values()))
    assert rec["cpus"] >= 1 and 0 <= rec["cpu_percent"] <= 100 * rec["cpus"]
    assert rec["mem"]["total"] > 0 and "gpus" in rec
    with urllib.request.urlopen(f"{base}/api/gpus", timeout=10) as r:
        assert isinstance(json.loads(r.read()), dict)
    with urllib.request.urlopen(f"{base}/api/nodes", timeout=10) as r:
        nodes = json.loads(r.read())
    assert any("physical_stats" in n for n in nodes)
    if logs:
        with urllib.request.urlopen(f"{base}/api/logs/{logs[0]}",
                                    timeout=10) as r:
            r.read()
    # metrics publish is fire-and-forget: retry the scrape
    deadline = time.time() + 15
    text = ""
    while time.time() < deadline:
        with urllib.request.urlopen(f"{base}/metrics", timeout=10) as r:
            text = r.read().decode()
        if 'test_requests_total{route="/a"} 3.0' in text:
            break
        time.sleep(0.5)
    assert 'test_requests_total{route="/a"} 3.0' in text
    assert "test_temp 42.5" in text
    assert 'test_lat_bucket{le="0.1"} 1' in text
    assert 'test_lat_bucket{le="+Inf"} 3' in text

    # job submission via REST
    req = urllib.request.Request(
        f"{base}/api/jobs",
        data=json.dumps({"entrypoint": "echo rest_job_ok"}).encode(),
        method="POST", headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=30) as r:
        sub = json.loads(r.read())
    job_id = sub["submission_id"]
    deadline = time.time() + 30
    while time.time() < deadline:
        with urllib.request.urlopen(f"{base}/api/jobs/{job_id}", timeout=10) as r:
            info = json.loads(r.read())
        if info.get("status") in ("SUCCEEDED", "FAILED"):
            break
        time.sleep(0.5)
    assert info["status"] == "SUCCEEDED"
    with urllib.request.urlopen(f"{base}/api/jobs/{job_id}/logs",
                                timeout=10) as r:
        assert b"rest_job_ok" in r.read()


def test_multiprocessing_pool(ray_mod):
    """ray.util.multiprocessing.Pool parity: map/starmap/apply_async/
    imap_unordered on actor-backed workers."""
    from ant_ray_amd.util.multiprocessing import Pool

    def sq(x):
        return x * x

    def add(a, b):
        return a + b

    with Pool(processes=3) as p:
        assert p.map(sq, range(10)) == [x * x for x in range(10)]
        assert p.starmap(add, [(1, 2), (3, 4)]) == [3, 7]
        ar = p.apply_async(sq, (9,))
        assert ar.get(timeout=60) == 81
        assert sorted(p.imap_unordered(sq, range(5))) == [0, 1, 4, 9, 16]
        assert list(p.imap(sq, range(5))) == [0, 1, 4, 9, 16]


def test_inspect_serializability():
    import threading

    from ant_ray_amd.util import inspect_serializability

    lk = threading.Lock()

    def bad():
        return lk

    ok, fails = inspect_serializability(bad)
    assert not ok and any("lk" in f for f in fails)
    ok, fails = inspect_serializability({"x": 1})
    assert ok and not fails


def test_kv_put_seq_ordering(ray_mod):
    """Regression: sequenced kv_put must reject stale overwrites so
    fire-and-forget metric publishes stay last-writer-wins even when the
    GCS handles them out of order (chaos-jitter repro)."""
    from ant_ray_amd._private.worker import global_worker

    cw = global_worker.core_worker

    def put(val, seq):
        return cw.io.submit(cw.gcs.call("kv_put", {
            "ns": "metrics", "key": b"seqtest",
            "value": val, "overwrite": True, "seq": seq,
        })).result(10)

    assert put(b"v1", 1)["added"]
    assert put(b"v3", 3)["added"]
    r = put(b"v2", 2)  # stale: must not win
    assert r.get("stale") or not r.get("added")
    got = cw.io.submit(cw.gcs.call("kv_get", {
        "ns": "metrics", "key": b"seqtest"})).result(10)
    assert got["value"] == b"v3"


def test_top_level_api_additions(ray_mod):
    """LoggingConfig / client builder / Language / show_in_dashboard /
    _config — top-level parity items (reference ray/__init__.py __all__)."""
    import io
    import logging

    import ant_ray_amd as ray

    # LoggingConfig validation + formatter behavior (no global apply here)
    from ant_ray_amd._private.logging_config import (CoreContextFilter,
                                                     JSONFormatter,
                                                     LoggingConfig)

    with pytest.raises(ValueError):
        LoggingConfig(encoding="YAML")
    with pytest.raises(ValueError):
        LoggingConfig(additional_log_standard_attrs=["nope"])
    lc = LoggingConfig(encoding="JSON", log_level="DEBUG",
                       additional_log_standard_attrs=["name"])
    rec = logging.LogRecord("t", logging.INFO, __file__, 1, "hello %s",
                            ("x",), None)
    CoreContextFilter().filter(rec)
    d = json.loads(JSONFormatter(["name"]).format(rec))
    assert d["message"] == "hello x" and d["name"] == "t"
    assert "worker_id" in d  # connected session stamps core context

    # Language / SCRIPT_MODE / xlang stubs
    assert ray.Language.PYTHON == "PYTHON"
    assert ray.SCRIPT_MODE == ray.DRIVER_MODE
    with pytest.raises(NotImplementedError):
        ray.java_function("C", "m")

    # client builder: on an already-initialized session connect() would
    # re-init; just exercise the builder plumbing + double-connect guard
    b = ray.client("127.0.0.1:9999").namespace("ns1").env({"env_vars": {}})
    assert b.address == "127.0.0.1:9999" and b._namespace == "ns1"

    # show_in_dashboard → /api/display
    ray.show_in_dashboard("working on shard 3", key="status")
    from ant_ray_amd.dashboard import start_dashboard

    port = start_dashboard(port=8277)  # idempotent if already started
    deadline = time.time() + 10
    disp = {}
    while time.time() < deadline:
        with urllib.request.urlopen(
                f"http://127.0.0.1:{port}/api/display", timeout=10) as r:
            disp = json.loads(r.read())
        if any(v.get("message") == "working on shard 3"
               for v in disp.values()):
            break
        time.sleep(0.2)
    assert any(v.get("message") == "working on shard 3"
               for v in disp.values()), disp

    # _config accessor
    assert callable(ray._config.some_unknown_flag)
    assert ray._config.some_unknown_flag(7) == 7


def test_util_parity_helpers(ray_mod):
    """as_completed / map_unordered / log_once / custom serializers /
    list_named_actors / get_placement_group (reference util/__init__.py
    surface)."""
    import ant_ray_amd as ray
    from ant_ray_amd.util import (as_completed, deregister_serializer,
                                  list_named_actors, map_unordered,
                                  register_serializer)
    from ant_ray_amd.util.debug import log_once, reset_log_once

    @ray.remote
    def sq(x):
        return x * x

    # as_completed yields everything, unordered
    refs = [sq.remote(i) for i in range(20)]
    assert sorted(as_completed(refs, chunk_size=4)) == [i * i for i in range(20)]
    # map_unordered with backpressure
    out = sorted(map_unordered(sq, range(25), backpressure_size=5,
                               chunk_size=3))
    assert out == [i * i for i in range(25)]

    # log_once
    reset_log_once("k1")
    assert log_once("k1") is True
    assert log_once("k1") is False

    # custom serializer round-trips through a task
    class Vec:
        def __init__(self, x, y):
            self.x, self.y = x, y

    register_serializer(Vec, serializer=lambda v: (v.x, v.y),
                        deserializer=lambda s: Vec(s[0] * 10, s[1] * 10))
    try:
        @ray.remote
        def through(v):
            return (v.x, v.y)

        assert ray.get(through.remote(Vec(1, 2)), timeout=30) == (10, 20)
    finally:
        deregister_serializer(Vec)

    # list_named_actors
    @ray.remote
    class Named:
        def ping(self):
            return "pong"

    a = Named.options(name="util_listed_actor").remote()
    ray.get(a.ping.remote(), timeout=30)
    assert "util_listed_actor" in list_named_actors()
    assert {"name": "util_listed_actor", "namespace": ""} in \
        list_named_actors(all_namespaces=True)
    ray.kill(a)

    # get_placement_group by name
    from ant_ray_amd.util import get_placement_group, placement_group, \
        remove_placement_group

    pg = placement_group([{"CPU": 1}], name="util_pg")
    assert pg.wait(30)
    found = get_placement_group("util_pg")
    assert found.id == pg.id
    remove_placement_group(pg)
    with pytest.raises(ValueError):
        get_placement_group("no_such_pg")


def test_logging_config_propagates_to_workers():
    """ray.init(logging_config=JSON) applies in SPAWNED WORKERS too: a
    task's log record comes out as JSON with core context (parity:
    reference logging_config propagation via runtime env)."""
    import subprocess
    import sys

    code = r"""
import ray
ray.init(num_cpus=1, logging_config=ray.LoggingConfig(encoding="JSON"))

@ray.remote
def noisy():
    import logging as L
    h = L.getLogger().handlers[-1]
    r = L.LogRecord("app", L.INFO, "t.py", 1, "probe %s", ("x",), None)
    for f in h.filters:
        f.filter(r)
    return h.format(r)

out = ray.get(noisy.remote(), timeout=60)
print("FORMATTED::" + out)
ray.shutdown()
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, timeout=180, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines()
            if ln.startswith("FORMATTED::")][0]
    payload = json.loads(line[len("FORMATTED::"):])
    assert payload["message"] == "probe x"
    assert "worker_id" in payload and "task_id" in payload
