"""Llama-3 family, MI355X-first implementation.

Design (not a port of any reference model code):
  * bf16 weights/activations; GEMMs via F.linear (hipBLASLt); everything
    memory-bound is a hand-written CDNA4 kernel (ant_ray_amd.ops):
      - fused residual-add + RMSNorm (one HBM pass)
      - RoPE applied IN PLACE on the fused QKV projection buffer (zero copies)
      - SwiGLU on the packed gate_up projection
      - chunked fused vocab-projection + cross-entropy (logits never
        materialize: 4.2 GB saved at B4xS4096xV128256)
  * attention: hand-written CDNA4 flash attention (ops.attention) on GPU for
    D=128; torch SDPA elsewhere — was: the
    next kernel on the roadmap
  * parameters live as views into flat buffers when wrapped by
    parallel.FlatParamManager (optimizer = one fused kernel pass).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ant_ray_amd import ops


@dataclass
class LlamaConfig:
    hidden: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 128
    intermediate: int = 14336
    vocab: int = 128256
    rope_theta: float = 500000.0
    max_seq: int = 4096
    eps: float = 1e-5
    tie_embeddings: bool = False

    @classmethod
    def llama3_8b(cls, max_seq=4096):
        return cls(max_seq=max_seq)

    @classmethod
    def tiny(cls, max_seq=512):
        return cls(hidden=256, n_layers=4, n_heads=4, n_kv_heads=2, head_dim=64,
                   intermediate=512, vocab=1024, max_seq=max_seq)


class KVCache:
    """Per-model KV cache for generation: [n_layers, B, Hk, max_seq, D]
    bf16, preallocated. `pos` = number of cached positions (uniform across
    the batch; ragged serve batches pass per-sequence lens to the decode
    kernel instead)."""

    def __init__(self, cfg: LlamaConfig, batch: int, max_seq: int, device):
        shape = (cfg.n_layers, batch, cfg.n_kv_heads, max_seq, cfg.head_dim)
        self.k = torch.empty(shape, device=device, dtype=torch.bfloat16)
        self.v = torch.empty(shape, device=device, dtype=torch.bfloat16)
        self.max_seq = max_seq
        self.pos = 0

    def layer(self, i: int):
        return self.k[i], self.v[i]

    def nbytes(self) -> int:
        return self.k.numel() * 2 * 2


class PagedKVCache:
    """Paged KV cache: page pools [n_layers, n_pages, Hk, P, D] bf16 plus a
    device block table int32 [slots, W] (layout documented at the top of
    csrc/kernels/attention_decode.hip). Key t of slot b lives at page
    block_table[b, t // P], slot t % P. Page 0 is the trash page that
    every unused table entry points at (llm/kv_blocks.py hands out pages
    1..n_pages-1). Passed as `cache` together with `lens`, the model runs
    the paged decode step; per-request prefill goes through seq_view()."""

    paged = True

    def __init__(self, cfg: LlamaConfig, n_pages: int, block_size: int,
                 slots: int, max_seq: int, device):
        shape = (cfg.n_layers, n_pages, cfg.n_kv_heads, block_size,
                 cfg.head_dim)
        self.k = torch.zeros(shape, device=device, dtype=torch.bfloat16)
        self.v = torch.zeros(shape, device=device, dtype=torch.bfloat16)
        self.block_size = block_size
        self.n_pages = n_pages
        self.max_seq = max_seq
        self.max_pages = -(-max_seq // block_size)
        self.block_table = torch.zeros(slots, self.max_pages,
                                       dtype=torch.int32, device=device)

    def layer(self, i: int):
        return self.k[i], self.v[i]

    def seq_view(self, pages) -> "PagedSeqCache":
        return PagedSeqCache(self, pages)

    def nbytes(self) -> int:
        return self.k.numel() * 2 * 2

    @staticmethod
    def page_bytes(cfg: LlamaConfig, block_size: int) -> int:
        return 2 * cfg.n_layers * cfg.n_kv_heads * block_size \
            * cfg.head_dim * 2


class PagedSeqCache:
    """One request's pages of a PagedKVCache, for prefill: write() stores a
    K/V span at its positions (torch index-copy; once per request, not the
    per-token path) and gather() returns a contiguous [1, Hk, n, D] copy
    of the first n positions (chunked prefill on a prefix hit). The flat
    pool-row index of a span is built once and reused by every layer."""

    paged = True

    def __init__(self, cache: PagedKVCache, pages):
        self.cache = cache
        self.P = cache.block_size
        self.pages = torch.as_tensor(pages, dtype=torch.long,
                                     device=cache.k.device)
        self._rows = {}

    def _index(self, pos: int, n: int):
        # rows of the layer pool viewed as [n_pages * Hk * P, D], ordered
        # [position, head]
        key = (pos, n)
        rows = self._rows.get(key)
        if rows is None:
            Hk = self.cache.k.shape[2]
            t = torch.arange(pos, pos + n, device=self.pages.device)
            base = self.pages[t // self.P] * Hk * self.P + t % self.P
            h = torch.arange(Hk, device=t.device) * self.P
            rows = (base[:, None] + h[None, :]).reshape(-1)
            self._rows[key] = rows
        return rows

    def write(self, i: int, pos: int, k, v) -> None:
        # k/v: [1, Hk, S, D] -> pool rows
        S, D = k.shape[2], k.shape[3]
        rows = self._index(pos, S)
        for pool, x in ((self.cache.k[i], k), (self.cache.v[i], v)):
            pool.view(-1, D).index_copy_(
                0, rows, x[0].transpose(0, 1).reshape(-1, D))

    def gather(self, i: int, n: int):
        D = self.cache.k.shape[-1]
        rows = self._index(0, n)
        out = []
        for pool in (self.cache.k[i], self.cache.v[i]):
            x = pool.view(-1, D).index_select(0, rows)
            out.append(x.view(n, -1, D).transpose(0, 1).unsqueeze(0)
                       .contiguous())
        return out[0], out[1]


class GraphedDecoder:
    """Persistent hipGraph-captured greedy decode loop for a FIXED
    (model, batch, cache): capture happens ONCE ever, then every token
    of every subsequent generate() on this decoder is one
    hipGraphLaunch. Serve replicas keep one per batch bucket
    (llm/native_engine.py) so repeated requests never pay capture or
    KV-cache allocation again. Requires head_dim 128 + CUDA + greedy."""

    def __init__(self, model: "LlamaForCausalLM", batch: int, max_seq: int,
                 device):
        self.model = model
        self.B = batch
        self.cache = KVCache(model.cfg, batch, max_seq, device)
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.cur = torch.zeros(batch, 1, dtype=torch.long, device=device)
        self.graph = None

    def _step(self):
        lg = self.model.forward(self.cur, cache=self.cache, lens=self.lens)
        self.cur.copy_(lg.argmax(dim=-1, keepdim=True))

    @torch.no_grad()
    def generate(self, tokens, max_new_tokens: int, prefix_len: int = 0):
        B, S = tokens.shape
        assert B == self.B, "decoder is fixed-batch; pad or re-bucket"
        # prefix_len > 0: cache[0:prefix_len) pre-seeded by the caller
        # (prefix-cache hit) — prefill only the suffix at pos=prefix_len
        logits = self.model.forward(
            tokens[:, prefix_len:] if prefix_len else tokens,
            cache=self.cache, pos=prefix_len)
        self.cache.pos = S
        self.lens.fill_(S)
        self.cur.copy_(logits.argmax(dim=-1, keepdim=True))
        out = [tokens]
        n_left = min(max_new_tokens, self.cache.max_seq - S + 1)
        emitted = 0
        while (emitted < n_left and self.graph is None and emitted < 2):
            out.append(self.cur.clone())
            emitted += 1
            if emitted >= n_left:
                break
            self.lens += 1
            self.cache.pos += 1
            self._step()
        if emitted < n_left and self.graph is None and n_left - emitted >= 8:
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                self.lens.add_(1)
                self._step()
            self.graph = g
        while emitted < n_left:
            out.append(self.cur.clone())
            emitted += 1
            if emitted >= n_left:
                break
            if self.graph is not None:
                self.graph.replay()
            else:
                self.lens += 1
                self._step()
            self.cache.pos += 1
        return torch.cat(out, dim=1)


class LlamaAttention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        Hq, Hk, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        self.wqkv = nn.Linear(cfg.hidden, (Hq + 2 * Hk) * D, bias=False)
        self.wo = nn.Linear(Hq * D, cfg.hidden, bias=False)

    def forward(self, y, cos, sin, cache=None, layer_idx=0, pos=0,
                lens=None):
        cfg = self.cfg
        Hq, Hk, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        B, S, _ = y.shape
        qkv = self.wqkv(y)
        if lens is not None:
            # graph-capturable decode step: position comes from the DEVICE
            # lens buffer (rope + cache write + flash-decode in one call —
            # no host scalar depends on the step index)
            ck, cv = cache.layer(layer_idx)
            if getattr(cache, "paged", False):
                o = ops.decode_step_attn_paged(
                    qkv.view(B, (Hq + 2 * Hk) * D), ck, cv,
                    cache.block_table, lens, cos, sin, Hq, Hk)
            else:
                o = ops.decode_step_attn(qkv.view(B, (Hq + 2 * Hk) * D), ck,
                                         cv, lens, cos, sin, Hq, Hk)
            return self.wo(o.view(B, 1, Hq * D))
        if (cache is None and qkv.is_cuda and D == 128
                and torch.is_grad_enabled() and qkv.requires_grad
                and os.environ.get("ANTRAY_FLASH", "1") != "0"):
            # training hot path: fused RoPE + flash attention with the
            # backward assembling dqkv in one buffer (no autograd
            # slice-scatter glue)
            o = ops.rope_attention(qkv, cos[pos : pos + S],
                                   sin[pos : pos + S], Hq, Hk, D,
                                   causal=True)
            o = o.transpose(1, 2).reshape(B, S, Hq * D)
            return self.wo(o)
        qkv = ops.rope_qkv(qkv, cos[pos : pos + S], sin[pos : pos + S],
                           Hq, Hk, D)
        q = qkv[..., : Hq * D].view(B, S, Hq, D).transpose(1, 2)
        k = qkv[..., Hq * D : (Hq + Hk) * D].view(B, S, Hk, D).transpose(1, 2)
        v = qkv[..., (Hq + Hk) * D :].view(B, S, Hk, D).transpose(1, 2)
        paged_fresh = False
        if cache is not None and getattr(cache, "paged", False):
            # paged prefill: the prompt's K/V goes into the request's
            # pages; a prefix hit gathers the pages into a temporary
            # contiguous buffer for the chunked-prefill path below, a cold
            # prompt attends over k/v straight from qkv
            cache.write(layer_idx, pos, k, v)
            if pos > 0:
                ck, cv = cache.gather(layer_idx, pos + S)
            else:
                paged_fresh = True
        elif cache is not None:
            ck, cv = cache.layer(layer_idx)
            ck[:, :, pos : pos + S] = k
            cv[:, :, pos : pos + S] = v
        if cache is not None and not paged_fresh:
            if S == 1:
                # single-token decode over the cache (flash-decode kernel)
                o = ops.attention_decode(q.reshape(B, Hq, D), ck, cv,
                                         seq_len=pos + 1)
                return self.wo(o.view(B, 1, Hq * D))
            if pos > 0:
                # chunked prefill (prefix-cache hit): queries at absolute
                # positions pos..pos+S-1 attend over cache[0:pos+S]
                # (prefix unmasked + suffix causal). GPU: suffix flash +
                # prefix GEMM/logsumexp, LSE-combined; CPU: masked SDPA.
                if qkv.is_cuda and D == 128 and os.environ.get(
                        "ANTRAY_FLASH", "1") != "0":
                    o = ops.chunked_prefill_attention(q, k, v, ck, cv, pos)
                else:
                    kf = ck[:, :, : pos + S]
                    vf = cv[:, :, : pos + S]
                    mask = torch.ones(S, pos + S, dtype=torch.bool,
                                      device=q.device).tril_(diagonal=pos)
                    o = F.scaled_dot_product_attention(
                        q, kf, vf, attn_mask=mask, enable_gqa=True)
                o = o.transpose(1, 2).reshape(B, S, Hq * D)
                return self.wo(o)
        if qkv.is_cuda and D == 128 and os.environ.get("ANTRAY_FLASH", "1") != "0":
            # hand-written CDNA4 flash attention — THE DEFAULT (fwd 1.30x
            # AOTriton at 514 TF/s, f+b 1.01x after the r2 instruction-diet
            # work: 64-key tiles, tr16 V reads with offset-immediates, raw
            # v_exp, Q pre-scale). ANTRAY_FLASH=0 falls back to SDPA.
            o = ops.attention(q, k, v, causal=True)
        else:
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True,
                                               enable_gqa=True)
        o = o.transpose(1, 2).reshape(B, S, Hq * D)
        return self.wo(o)


class LlamaMLP(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.w_gate_up = nn.Linear(cfg.hidden, 2 * cfg.intermediate, bias=False)
        self.w_down = nn.Linear(cfg.intermediate, cfg.hidden, bias=False)

    def forward(self, y):
        return self.w_down(ops.swiglu(self.w_gate_up(y)))


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.attn_norm = nn.Parameter(torch.ones(cfg.hidden))
        self.mlp_norm = nn.Parameter(torch.ones(cfg.hidden))
        self.attn = LlamaAttention(cfg)
        self.mlp = LlamaMLP(cfg)

    def forward(self, h, res, cos, sin, cache=None, layer_idx=0, pos=0,
                lens=None):
        # h = contribution from the previous sublayer; res = residual stream
        if res is None:
            res = h
            y = ops.rmsnorm(h, self.attn_norm, self.cfg.eps)
        else:
            y, res = ops.fused_add_rmsnorm(h, res, self.attn_norm, self.cfg.eps)
        a = self.attn(y, cos, sin, cache=cache, layer_idx=layer_idx, pos=pos,
                      lens=lens)
        y2, res = ops.fused_add_rmsnorm(a, res, self.mlp_norm, self.cfg.eps)
        return self.mlp(y2), res


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: LlamaConfig, device=None):
        super().__init__()
        self.cfg = cfg
        factory = {"device": device, "dtype": torch.bfloat16}
        with torch.device(device or "cpu"):
            self.embed = nn.Embedding(cfg.vocab, cfg.hidden)
            self.blocks = nn.ModuleList(LlamaBlock(cfg) for _ in range(cfg.n_layers))
            self.final_norm = nn.Parameter(torch.ones(cfg.hidden))
            if cfg.tie_embeddings:
                self.lm_head = None
            else:
                self.lm_head = nn.Linear(cfg.hidden, cfg.vocab, bias=False)
        self.to(dtype=torch.bfloat16)
        if device is not None:
            self.to(device)
        self._init_weights()
        cos, sin = ops.rope_tables(cfg.head_dim, cfg.max_seq, cfg.rope_theta,
                                   device=device or "cpu")
        self.register_buffer("rope_cos", cos, persistent=False)
        self.register_buffer("rope_sin", sin, persistent=False)

    def _init_weights(self):
        std = 0.02
        out_std = std / math.sqrt(2 * self.cfg.n_layers)
        for name, p in self.named_parameters():
            if p.dim() >= 2:
                s = out_std if ("wo" in name or "w_down" in name) else std
                nn.init.normal_(p, mean=0.0, std=s)

    @property
    def head_weight(self):
        return self.embed.weight if self.lm_head is None else self.lm_head.weight

    def forward(self, tokens, targets=None, cache=None, pos=0, lens=None):
        B, S = tokens.shape
        h = self.embed(tokens)
        res = None
        cos, sin = self.rope_cos, self.rope_sin
        for i, blk in enumerate(self.blocks):
            h, res = blk(h, res, cos, sin, cache=cache, layer_idx=i, pos=pos,
                         lens=lens)
        if res is None:
            y = ops.rmsnorm(h, self.final_norm, self.cfg.eps)
        else:
            y, _ = ops.fused_add_rmsnorm(h, res, self.final_norm, self.cfg.eps)
        if cache is not None and targets is None:
            # generation: logits only for the LAST position (saves the
            # full-sequence vocab projection on prefill)
            y_last = y[:, -1, :]
            return y_last @ self.head_weight.t()
        flat = y.reshape(B * S, self.cfg.hidden)
        if targets is not None:
            return ops.linear_cross_entropy(flat, self.head_weight, targets.reshape(-1))
        return (flat @ self.head_weight.t()).view(B, S, -1)

    @torch.no_grad()
    def generate(self, tokens, max_new_tokens: int, cache: "KVCache" = None,
                 temperature: float = 0.0, start_pos: int = 0):
        """Greedy (temperature=0) or sampled generation with the KV cache +
        flash-decode kernel. tokens: [B, S_prompt] int64. Returns
        [B, S_prompt + max_new_tokens].

        start_pos > 0 = prefix-cache hit: positions [0, start_pos) of
        `cache` were seeded by the caller (llm/prefix_cache.py) and only
        tokens[:, start_pos:] are prefilled (chunked prefill).

        Role parity: the reference serves generation through vLLM
        (reference python/ray/llm/_internal/serve/engines/vllm/
        vllm_engine.py:1); this is the in-tree MI355X-native decode loop
        used by the framework's own Serve LLM path."""
        B, S = tokens.shape
        dev = tokens.device
        if cache is None:
            cache = KVCache(self.cfg, B, min(self.cfg.max_seq,
                                             S + max_new_tokens), dev)
        logits = self.forward(tokens[:, start_pos:] if start_pos else tokens,
                              cache=cache, pos=start_pos)  # prefill
        cache.pos = S
        use_graph = (tokens.is_cuda and self.cfg.head_dim == 128
                     and temperature == 0
                     and os.environ.get("ANTRAY_DECODE_GRAPH", "1") != "0")
        if use_graph:
            return self._generate_graphed(tokens, logits, cache,
                                          max_new_tokens)
        out = [tokens]
        cur = None
        for _ in range(max_new_tokens):
            if temperature > 0:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                cur = torch.multinomial(probs, 1)
            else:
                cur = logits.argmax(dim=-1, keepdim=True)
            out.append(cur)
            if cache.pos >= cache.max_seq:
                break
            logits = self.forward(cur, cache=cache, pos=cache.pos)
            cache.pos += 1
        return torch.cat(out, dim=1)

    @torch.no_grad()
    def _generate_graphed(self, tokens, logits, cache: "KVCache",
                          max_new_tokens: int):
        """Greedy decode with the whole token step captured in a hipGraph.

        The device-pos decode path (ops.decode_step_attn: rope + cache
        write + flash-decode reading pos from the device lens buffer)
        makes every kernel argument independent of the step index, so
        ONE capture serves all steps: each replay advances `cur` (next
        token) and `lens` in place on the GPU. The eager host-pos loop
        pays ~260 Python-side launches per token; the replay is one
        hipGraphLaunch. Capture happens once per (B, cache) generate
        call (first token runs eagerly as the capture warmup)."""
        B, S = tokens.shape
        dev = tokens.device
        lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        cur = logits.argmax(dim=-1, keepdim=True)  # token 1 (from prefill)
        out = [tokens]
        n_left = min(max_new_tokens, cache.max_seq - S + 1)

        def step():
            lg = self.forward(cur, cache=cache, lens=lens)
            cur.copy_(lg.argmax(dim=-1, keepdim=True))

        emitted = 0
        # warmup steps run eagerly (they also produce real tokens)
        for _ in range(min(2, n_left)):
            out.append(cur.clone())
            emitted += 1
            if emitted >= n_left:
                break
            lens += 1
            cache.pos += 1
            step()
        if emitted < n_left and n_left - emitted >= 8:
            # capture costs ~10s of ms once; only worth it for a real run
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                lens.add_(1)
                step()
            # capture records without executing: lens/cur are unchanged
            while emitted < n_left:
                out.append(cur.clone())
                emitted += 1
                if emitted >= n_left:
                    break
                g.replay()
                cache.pos += 1
        else:
            while emitted < n_left:
                out.append(cur.clone())
                emitted += 1
                if emitted >= n_left:
                    break
                lens += 1
                cache.pos += 1
                step()
        return torch.cat(out, dim=1)

    def num_params(self):
        return sum(p.numel() for p in self.parameters())
