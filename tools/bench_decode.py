"""Decode-path benchmarks on the GPU box.

1. attn_decode kernel: ms + achieved GB/s of KV-cache read at llama3-8b
   decode shapes (the kernel is memory-bound; ceiling ~6.3 TB/s).
1b. paged vs contiguous: the paged kernel (block table over a shuffled
   page order, --block-size tokens per page) and the contiguous kernel on
   the same K/V, timed in the same process, alternating rounds. Bytes
   are computed from shapes (K+V rows read), identical for both.
2. end-to-end generate() tokens/s for llama3-8b bf16 at a few batch sizes
   (weights 16 GB re-read per step -> ~2.5 ms/step floor at the HBM
   ceiling, plus KV bytes).

Run: python tools/bench_decode.py [--model llama3-8b] [--paged-only]
     [--block-size 64] [--json-out profiles/decode_paged.json]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import ant_ray_amd.ops as ops


def bench(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / iters


def paged_rows(args):
    """Paged vs contiguous decode kernel at the same shapes, alternating
    A/B rounds in one process; per-call time = median round."""
    import json
    import statistics

    P = args.block_size
    Hq, Hk, D = 32, 8, 128
    print(f"== paged vs contiguous attn_decode (P={P}, shuffled pages) ==")
    rows = []
    for B, T in [(1, 1024), (1, 4096), (8, 1024), (8, 4096), (32, 2048),
                 (64, 4096)]:
        W = T // P
        q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Hk, T, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, Hk, T, D, device="cuda", dtype=torch.bfloat16)
        lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
        table = (torch.randperm(B * W, device="cuda") + 1).view(B, W)
        kp = torch.zeros(B * W + 1, Hk, P, D, device="cuda",
                         dtype=torch.bfloat16)
        vp = torch.zeros_like(kp)
        kp[table.reshape(-1)] = k.view(B, Hk, W, P, D).permute(
            0, 2, 1, 3, 4).reshape(B * W, Hk, P, D)
        vp[table.reshape(-1)] = v.view(B, Hk, W, P, D).permute(
            0, 2, 1, 3, 4).reshape(B * W, Hk, P, D)
        table = table.to(torch.int32).contiguous()
        o_c = ops.attention_decode(q, k, v, seq_len=T, lens=lens)
        o_p = ops.attention_decode_paged(q, kp, vp, table, lens)
        err = (o_c.float() - o_p.float()).abs().max().item()
        tc, tp = [], []
        for _ in range(args.rounds):
            tc.append(bench(lambda: ops.attention_decode(
                q, k, v, seq_len=T, lens=lens)))
            tp.append(bench(lambda: ops.attention_decode_paged(
                q, kp, vp, table, lens)))
        t_c, t_p = statistics.median(tc), statistics.median(tp)
        bytes_rd = B * Hk * T * D * 2 * 2
        row = {"B": B, "T": T, "P": P,
               "contig_us": round(t_c * 1e6, 2),
               "paged_us": round(t_p * 1e6, 2),
               "contig_TBps": round(bytes_rd / t_c / 1e12, 3),
               "paged_TBps": round(bytes_rd / t_p / 1e12, 3),
               "paged_over_contig": round(t_c / t_p, 3),
               "max_abs_diff": err}
        rows.append(row)
        print(f"B={B:3d} T={T:5d}: contig {t_c*1e6:8.1f} us "
              f"{row['contig_TBps']:5.2f} TB/s | paged {t_p*1e6:8.1f} us "
              f"{row['paged_TBps']:5.2f} TB/s | ratio "
              f"{row['paged_over_contig']:.3f} | max|diff| {err:.3g}",
              flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump({"metric": "attn_decode paged vs contiguous "
                       "(llama3-8b heads, same process, alternating)",
                       "bytes": "B*Hk*T*D*2 (K+V) bf16, from shapes",
                       "rounds": args.rounds, "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--gen-batches", default="1,8,32")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--block-size", type=int, default=64)
    ap.add_argument("--paged-only", action="store_true",
                    help="kernel rows only (skip the generate() section)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json-out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py needs a GPU")

    print("== attn_decode kernel (llama3-8b shapes) ==")
    Hq, Hk, D = 32, 8, 128
    for B, T in [(1, 1024), (1, 4096), (8, 1024), (8, 4096), (32, 2048)]:
        q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Hk, T, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, Hk, T, D, device="cuda", dtype=torch.bfloat16)
        t = bench(lambda: ops.attention_decode(q, k, v, seq_len=T))
        bytes_rd = B * Hk * T * D * 2 * 2
        print(f"B={B:3d} T={T:5d}: {t*1e6:8.1f} us  {bytes_rd/t/1e12:6.2f} TB/s")

    paged_rows(args)
    if args.paged_only:
        return

    print(f"== generate() {args.model} ==")
    from ant_ray_amd.models import build_model, setup_tunableop

    setup_tunableop()

    m = build_model(args.model, device="cuda",
                    seq_len=args.prompt + args.new_tokens + 8)
    m.eval()
    vocab = m.cfg.vocab
    for B in [int(x) for x in args.gen_batches.split(",")]:
        toks = torch.randint(0, vocab, (B, args.prompt), device="cuda")
        # warm — 12 new tokens crosses the graph-capture threshold so the
        # process's expensive FIRST hipGraph instantiation (~0.7 s) lands
        # here, not in the timed region
        m.generate(toks[:, :32], max_new_tokens=12)
        torch.cuda.synchronize()
        t0 = time.time()
        out = m.generate(toks, max_new_tokens=args.new_tokens)
        torch.cuda.synchronize()
        wall = time.time() - t0
        ntok = out.shape[1] - args.prompt
        print(f"B={B:3d}: prefill+{ntok} new in {wall*1e3:8.1f} ms  "
              f"decode {B*ntok/wall:8.1f} tok/s  "
              f"({wall/ntok*1e3:6.2f} ms/step incl prefill amortized)")


if __name__ == "__main__":
    main()
