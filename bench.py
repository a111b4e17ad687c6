"""Flagship benchmark: tokens/sec, Llama-3-8B Ray Train DDP (BASELINE.json).

Default path (--via-ray, on): the measured number is produced by an actual
Ray Train run — ray.init + TorchTrainer + placement group pinning one
worker actor per GPU — the same stack a user of the framework runs
(parity: reference python/ray/train/v2/api/data_parallel_trainer.py:155).
The training engine inside each worker is FlatDDP (bucketed RCCL
all-reduce overlapped with backward) + fused flat AdamW on the CDNA4 HIP
kernels. `--bare` keeps the round-1 no-runtime path for A/B overhead
checks (tools/bench_parity.py measures the delta).

Launch contract (driver): N=1 is `python bench.py --gpus 1 ...`; N>1 is
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
Under torchrun, only RANK 0 proceeds in via-ray mode (it drives the Ray
cluster that spawns one worker actor per GPU); other ranks exit 0
immediately without touching the GPU. In --bare mode every rank is a DDP
rank as in round 1.

Timing: W untimed warmup steps, then exactly K steps bracketed by
barrier+synchronize on both sides, elapsed MAX-reduced over ranks, ONE
JSON line from rank 0 with the whole-job aggregate tokens/s.

--dump-outputs DIR: after the timed window, rank 0 writes what the last
timed step produced as DIR/<name>.npy (see _dump_outputs). Inputs are
seeded, so two builds run with the same arguments can be compared
output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import time

# per-array cap on the sampled flat-buffer elements written by
# --dump-outputs: 3 fp32 arrays x 4M = 48 MB, under the 64 MB budget
DUMP_SAMPLE = 4 << 20
DUMP_SEED = 0


def _setup_tunableop(local_rank: int):
    """hipBLASLt algo selection via torch TunableOp: load the committed
    pre-tuned table for the model's GEMM shapes (profiles/tunableop_gfx950
    .csv, measured +4-8% over the default heuristics on gfx950); set
    ANTRAY_TUNE=1 to (re)tune and write a fresh table."""
    if os.environ.get("ANTRAY_TUNEOP") == "0":
        # TunableOp's hipblasLtCreate aborts under rocprofv3 counter
        # collection — profiling runs disable it
        return
    try:
        import torch.cuda.tunable as tun
    except ImportError:
        return
    here = os.path.dirname(os.path.abspath(__file__))
    table = os.path.join(here, "profiles", "tunableop_gfx950.csv")
    tuning = os.environ.get("ANTRAY_TUNE") == "1"
    if not tuning and not os.path.exists(table):
        return
    tun.enable(True)
    out = os.environ.get("ANTRAY_TUNE_OUT",
                         f"/tmp/tunableop_rank{local_rank}.csv")
    tun.set_filename(out if tuning else table)
    if tuning:
        if os.path.exists(table):
            try:
                tun.read_file(table)  # only UNSEEN shapes get tuned
            except Exception:
                pass
        tun.tuning_enable(True)
        tun.set_max_tuning_duration(100)
    else:
        tun.tuning_enable(False)
        try:
            tun.read_file(table)
        except Exception:
            pass


def _parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch size")
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--bucket-mb", type=int, default=64)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--bare", action="store_true",
                    help="skip the Ray runtime: raw torchrun DDP ranks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/*.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.dump_outputs:
        # Ray worker actors do not share the driver's cwd
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    return args


def _resolve_batch(args) -> int:
    if args.model.startswith("gpt2"):
        args.seq = min(args.seq, 1024)
        return args.batch or 16
    # batch 6 x seq 4096 ~ 250 GB of 288 GB HBM (measured): biggest safe
    # per-GPU batch with headroom for RCCL workspaces at 8 GPUs
    return args.batch or 6


def _train_core(args, device, rank: int, world: int):
    """The measured loop, identical for both paths. Requires the process
    group to already exist when world > 1. Returns (elapsed_s, loss)."""
    import torch

    on_gpu = str(device).startswith("cuda")

    from ant_ray_amd.models import build_model
    from ant_ray_amd.parallel import FlatAdamW, FlatDDP, FlatParamManager

    batch = _resolve_batch(args)
    torch.manual_seed(1234 + rank)
    t_build = time.time()
    model = build_model(args.model, device=device, seq_len=args.seq)
    mgr = FlatParamManager(model, device=device)
    ddp = FlatDDP(model, manager=mgr, bucket_mb=args.bucket_mb)
    opt = FlatAdamW(mgr, lr=args.lr, weight_decay=0.1)
    vocab = model.cfg.vocab
    if rank == 0:
        print(
            f"# model={args.model} params={model.num_params()/1e9:.2f}B "
            f"world={world} batch/gpu={batch} seq={args.seq} "
            f"build={time.time()-t_build:.1f}s",
            flush=True,
        )

    def step():
        tokens = torch.randint(0, vocab, (batch, args.seq), device=device)
        targets = torch.randint(0, vocab, (batch, args.seq), device=device)
        loss = ddp(tokens, targets)
        loss.backward()
        ddp.finish_grad_sync()
        opt.step()
        opt.zero_grad()
        return loss

    import torch.distributed as dist

    for _ in range(args.warmup):
        loss = step()
    if world > 1:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        loss = step()
    if on_gpu:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.time() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, loss, opt)
    return elapsed, float(loss.item())


def _dump_outputs(out_dir: str, loss, opt):
    """What a timed step hands back: its loss, and the weights and AdamW
    moments it updated (the moments carry the gradients, which the step
    zeroes at its end). The flat buffers are gathered at a fixed seeded
    set of at most DUMP_SAMPLE indices, the same for every run of the
    same model."""
    import numpy as np
    import torch

    numel = opt.master.numel()
    if numel <= DUMP_SAMPLE:
        idx = torch.arange(numel)
    else:
        gen = torch.Generator().manual_seed(DUMP_SEED)
        idx = torch.randint(0, numel, (DUMP_SAMPLE,), generator=gen).sort().values
    idx = idx.to(opt.master.device)
    arrays = {
        "loss": loss.detach().double().reshape(1),
        "params": opt.master[idx],
        "exp_avg": opt.m[idx],
        "exp_avg_sq": opt.v[idx],
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def _emit(args, world: int, elapsed: float, final_loss: float):
    batch = _resolve_batch(args)
    tokens_total = batch * args.seq * args.steps * world
    out = {
        "metric": "tokens/sec Llama-3-8B Ray Train DDP"
        if not args.model.startswith("gpt2")
        else "tokens/sec GPT-2-small DDP",
        "value": round(tokens_total / elapsed, 1),
        "unit": "tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1000, 2),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic",
        "config": {
            "model": args.model,
            "global_batch": batch * world,
            "seq_len": args.seq,
            "parallelism": f"dp{world}",
            "via": "bare-torchrun" if args.bare else "ray-train",
            "final_loss": round(final_loss, 4),
        },
    }
    print(json.dumps(out), flush=True)


def _main_bare(args):
    import torch

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(backend="nccl", rank=rank, world_size=world)
    device = f"cuda:{local_rank}"
    _setup_tunableop(local_rank)
    elapsed, final_loss = _train_core(args, device, rank, world)
    if rank == 0:
        _emit(args, world, elapsed, final_loss)
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


def _train_fn(config):
    """Runs inside each Ray Train worker actor (1 GPU each)."""
    import torch

    from ant_ray_amd import train

    args = argparse.Namespace(**config)
    ctx = train.get_context()
    rank = ctx.get_world_rank()
    world = ctx.get_world_size()
    device = train.torch.get_device()
    if str(device).startswith("cuda"):
        torch.cuda.set_device(device)
        _setup_tunableop(ctx.get_local_rank())
    elapsed, final_loss = _train_core(args, str(device), rank, world)
    train.report({"elapsed": elapsed, "final_loss": final_loss,
                  "world": world})


def _main_via_ray(args):
    # Under torchrun only rank 0 drives the Ray cluster; sibling ranks
    # exit clean without touching the GPU (the worker ACTORS are the
    # ranks). torchrun waits for all workers, so the early exits are fine.
    if int(os.environ.get("RANK", 0)) != 0:
        return
    # the worker group does its own rendezvous on a free port; drop the
    # torchrun-provided one so nothing collides with it
    for k in list(os.environ):
        if k in ("MASTER_ADDR", "MASTER_PORT", "RANK", "LOCAL_RANK",
                 "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK",
                 "NODE_RANK", "ROLE_RANK", "ROLE_WORLD_SIZE",
                 "ROLE_NAME") or k.startswith("TORCHELASTIC"):
            # TORCHELASTIC_USE_AGENT_STORE=True makes every descendant's
            # init_process_group try to JOIN torchrun's agent store at
            # MASTER_PORT instead of creating its own -> the worker
            # actors' gloo/nccl rendezvous hangs forever
            os.environ.pop(k, None)

    import ant_ray_amd as ray
    from ant_ray_amd.train import RunConfig, ScalingConfig
    from ant_ray_amd.train.torch import TorchTrainer

    n = args.gpus
    # ANTRAY_BENCH_CPU=1: plumbing-test mode — same torchrun->rank0->ray->
    # TorchTrainer shape on CPU/gloo with a tiny model (CI covers the
    # exact launch path the driver uses for the N>1 scaling bench)
    cpu_mode = os.environ.get("ANTRAY_BENCH_CPU") == "1"
    ray.init(num_cpus=max(8, 2 * n), num_gpus=0 if cpu_mode else n)
    try:
        trainer = TorchTrainer(
            _train_fn,
            train_loop_config=dict(vars(args)),
            scaling_config=ScalingConfig(num_workers=n,
                                         use_gpu=not cpu_mode),
            run_config=RunConfig(name="bench", storage_path="/tmp/antray_bench"),
        )
        result = trainer.fit()
        if result.error is not None:
            raise result.error
        m = result.metrics
        _emit(args, int(m["world"]), float(m["elapsed"]),
              float(m["final_loss"]))
    finally:
        ray.shutdown()


def main():
    args = _parse_args()
    if args.bare:
        _main_bare(args)
    else:
        _main_via_ray(args)


if __name__ == "__main__":
    main()
