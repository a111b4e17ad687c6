"""Serve LLM benchmark (BASELINE config 4, measured at the replicas a
1-GPU lease allows): Llama-3-8B bf16 behind a Serve deployment with the
native MI355X engine, dynamic batching, measured req/s + latency
percentiles. Writes profiles/serve_llama3_8b_<n>gpu_r02.json via --out.

Run on the GPU box:
  python tools/bench_serve_llm.py [--model llama3-8b] [--replicas 1]
      [--requests 64] [--concurrency 16] [--prompt 128] [--new-tokens 32]
      [--continuous [--paged-kv --block-size 64 --kv-cache-mb N]]
      [--max-model-len L] [--long-mix]

--long-mix sends ragged short prompts plus --long-count prompts of
--long-len tokens (spread evenly through the run) — the capacity shape a
contiguous KV cache cannot hold at long max_model_len.

With --in-process the continuous engine runs in this process instead of
behind Serve, so the paged pool's page counts and
torch.cuda.max_memory_allocated() can be reported.
"""
import argparse
import json
import os
import random
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _summary(args, max_len, lat, wall, n_req):
    lat = sorted(lat)
    n = len(lat)
    return {
        "model": args.model,
        "requests": n_req,
        "completed": n,
        "concurrency": args.concurrency,
        "prompt_tokens": args.prompt,
        "new_tokens": args.new_tokens,
        "req_per_s": round(n / wall, 3),
        "gen_tok_per_s": round(n * args.new_tokens / wall, 1),
        "p50_s": round(lat[n // 2], 3) if n else None,
        "p95_s": round(lat[min(n - 1, int(n * 0.95))], 3) if n else None,
        "wall_s": round(wall, 2),
        "continuous_batching": True,
        "ragged_prompts": args.ragged,
        "paged_kv": args.paged_kv,
        "block_size": args.block_size if args.paged_kv else None,
        "max_model_len": max_len,
        "long_mix": args.long_mix,
        "long_len": args.long_len if args.long_mix else None,
        "long_count": args.long_count if args.long_mix else None,
    }


def run_in_process(args, max_len, req_payload):
    """Continuous engine in this process (no Serve hop): the same
    closed-loop load at --concurrency, plus page-pool stats and peak
    device memory."""
    import torch

    from ant_ray_amd.llm.continuous import ContinuousLLMEngine

    eng = ContinuousLLMEngine(
        args.model, slots=args.concurrency, max_seq=max_len,
        device=args.device, start_thread=True,
        kv_cache="paged" if args.paged_kv else "contiguous",
        block_size=args.block_size, kv_pool_mb=args.kv_cache_mb)
    try:
        warm = req_payload()
        eng.submit(warm["prompt_ids"], warm["max_new_tokens"]).result(
            timeout=600)
        lat = []
        lock = threading.Lock()
        sem = threading.Semaphore(args.concurrency)
        futs = []
        t_start = time.time()
        for _ in range(args.requests):
            sem.acquire()
            pl = req_payload()
            t0 = time.time()
            fut = eng.submit(pl["prompt_ids"], pl["max_new_tokens"])

            def done(f, t0=t0):
                with lock:
                    lat.append(time.time() - t0)
                sem.release()

            fut.add_done_callback(done)
            futs.append(fut)
        for f in futs:
            f.result(timeout=1800)
        wall = time.time() - t_start
        st = eng.stats()
        res = _summary(args, max_len, lat, wall, args.requests)
        res.update({
            "metric": "continuous engine in-process req/s",
            "engine_stats": st,
            "kv_bytes": eng.dec.cache.nbytes(),
            "max_memory_allocated_bytes": (
                torch.cuda.max_memory_allocated()
                if args.device.startswith("cuda") else None),
            "contiguous_kv_bytes_computed": (
                2 * eng.model.cfg.n_layers * eng.model.cfg.n_kv_heads
                * eng.model.cfg.head_dim * 2 * args.concurrency * max_len),
        })
    finally:
        eng.shutdown()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--concurrency", type=int, default=16)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--out", default="")
    ap.add_argument("--continuous", action="store_true",
                    help="token-level continuous batching engine")
    ap.add_argument("--ragged", action="store_true",
                    help="sample prompt lengths in [16, --prompt] instead "
                         "of fixed (exposes batching-policy differences)")
    ap.add_argument("--paged-kv", action="store_true",
                    help="paged KV cache (continuous engine only)")
    ap.add_argument("--block-size", type=int, default=64)
    ap.add_argument("--kv-cache-mb", type=float, default=None,
                    help="paged KV pool size (MiB)")
    ap.add_argument("--max-model-len", type=int, default=0,
                    help="engine max_seq (default prompt + new + 8)")
    ap.add_argument("--long-mix", action="store_true",
                    help="ragged short prompts plus a few long ones")
    ap.add_argument("--long-len", type=int, default=24576)
    ap.add_argument("--long-count", type=int, default=2)
    ap.add_argument("--in-process", action="store_true",
                    help="drive ContinuousLLMEngine directly (reports "
                         "page stats and peak device memory)")
    ap.add_argument("--device", default="cuda",
                    help="--in-process device (cpu only for rehearsal)")
    args = ap.parse_args()
    max_len = args.max_model_len or args.prompt + args.new_tokens + 8
    if args.paged_kv and not args.continuous:
        ap.error("--paged-kv requires --continuous")
    if args.in_process and not args.continuous:
        ap.error("--in-process drives the continuous engine")
    vocab = 128256 if "8b" in args.model else 1024
    rng = random.Random(0)
    long_at = set()
    if args.long_mix and args.long_count:
        step = max(1, args.requests // args.long_count)
        long_at = {i * step + step // 2 for i in range(args.long_count)}
    counter = [0]
    counter_lock = threading.Lock()

    def req_payload():
        with counter_lock:
            i = counter[0]
            counter[0] += 1
        if i - 1 in long_at:  # payload 0 is the warmup request
            plen = args.long_len
        elif args.ragged or args.long_mix:
            plen = rng.randrange(16, args.prompt + 1)
        else:
            plen = args.prompt
        return {"prompt_ids": [rng.randrange(vocab) for _ in range(plen)],
                "max_new_tokens": args.new_tokens}

    if args.in_process:
        return run_in_process(args, max_len, req_payload)

    import ant_ray_amd as ray
    from ant_ray_amd import serve
    from ant_ray_amd.llm import LLMConfig, build_llm_deployment

    ray.init(num_cpus=8, num_gpus=args.replicas)
    app = build_llm_deployment(LLMConfig(
        model_loading_config={"model_id": args.model},
        engine_kwargs={"max_model_len": max_len,
                       "max_num_seqs": args.concurrency,
                       "continuous_batching": args.continuous,
                       "paged_kv": args.paged_kv,
                       "block_size": args.block_size,
                       "kv_cache_memory_mb": args.kv_cache_mb},
        deployment_config={"num_replicas": args.replicas},
    ))
    h = serve.run(app, name="llm", route_prefix="/llm")

    # warm (model build + first kernels)
    r = h.remote(req_payload()).result(timeout_s=600)
    assert len(r["token_ids"]) == args.new_tokens, r

    lat = []
    lat_lock = threading.Lock()
    sem = threading.Semaphore(args.concurrency)
    done = threading.Event()
    remaining = [args.requests]

    def fire():
        t0 = time.time()
        resp = h.remote(req_payload())

        def wait():
            try:
                resp.result(timeout_s=600)
                with lat_lock:
                    lat.append(time.time() - t0)
            finally:
                sem.release()
                with lat_lock:
                    remaining[0] -= 1
                    if remaining[0] == 0:
                        done.set()

        threading.Thread(target=wait, daemon=True).start()

    t_start = time.time()
    for _ in range(args.requests):
        sem.acquire()
        fire()
    done.wait(timeout=900)
    wall = time.time() - t_start

    lat.sort()
    n = len(lat)
    result = {
        "metric": "Serve Llama-3-8B bf16 req/s (native engine)",
        "model": args.model,
        "replicas": args.replicas,
        "requests": args.requests,
        "concurrency": args.concurrency,
        "prompt_tokens": args.prompt,
        "new_tokens": args.new_tokens,
        "req_per_s": round(n / wall, 3),
        "gen_tok_per_s": round(n * args.new_tokens / wall, 1),
        "p50_s": round(lat[n // 2], 3) if n else None,
        "p95_s": round(lat[int(n * 0.95)] if n > 1 else lat[0], 3) if n else None,
        "wall_s": round(wall, 2),
        "completed": n,
        "continuous_batching": args.continuous,
        "ragged_prompts": args.ragged,
        "paged_kv": args.paged_kv,
        "block_size": args.block_size if args.paged_kv else None,
        "max_model_len": max_len,
        "long_mix": args.long_mix,
    }
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    serve.shutdown()
    ray.shutdown()


if __name__ == "__main__":
    main()
