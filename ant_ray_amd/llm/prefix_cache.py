"""Hash-based block prefix caching for the native LLM engine.

Role parity: vLLM's automatic prefix caching, which the reference exposes
through its engine kwargs (reference python/ray/llm/_internal/serve/
engines/vllm/vllm_engine.py:1). Design here is MI355X-native: the decode
kernels (csrc/kernels/attention_decode.hip) read CONTIGUOUS per-request
KV caches in the default engines, so prefix reuse is done by COPY (the
continuous engine's opt-in paged mode shares prefix pages by reference
instead: llm/kv_blocks.py): cached prompt-prefix KV
blocks are device-to-device copied into the decoder's contiguous cache
(a few MB over an ~8 TB/s fabric, microseconds) and only the prompt
suffix is prefilled (chunked prefill in models/llama.py). What is saved
is the prefill FLOPs of the shared prefix — the expensive part for long
shared system prompts / multi-turn contexts.

Keying matches vLLM's scheme: a prompt is split into fixed-size token
blocks; each block's key is a rolling hash of the whole token chain up to
and including that block, so a block is reusable only when EVERYTHING
before it matches. Entries verify the exact token prefix on lookup (hash
collisions cannot alias). Eviction is LRU under a byte budget.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import torch


@dataclass
class _Block:
    prefix: tuple          # exact token chain up to and incl. this block
    k: torch.Tensor        # [n_layers, Hk, block_size, D] bf16
    v: torch.Tensor


class PrefixKVCache:
    """In-process (per-replica) prefix KV block cache.

    block_size: tokens per block (hits are block-granular).
    budget_mb: LRU byte budget for stored K+V blocks.
    """

    def __init__(self, block_size: int = 64, budget_mb: float = 512.0):
        self.bs = int(block_size)
        self.budget = int(budget_mb * (1 << 20))
        self._blocks: "OrderedDict[int, _Block]" = OrderedDict()
        self._bytes = 0
        self.hits = 0
        self.misses = 0
        self.tokens_reused = 0

    # ------------------------------------------------------------- keys
    def _chain_keys(self, tokens: Sequence[int]) -> List[Tuple[int, tuple]]:
        """[(rolling_key, block_tokens), ...] for each full block."""
        out = []
        chain = 0
        for i in range(len(tokens) // self.bs):
            blk = tuple(tokens[i * self.bs : (i + 1) * self.bs])
            chain = hash((chain, blk))
            out.append((chain, blk))
        return out

    # ----------------------------------------------------------- lookup
    def lookup(self, tokens: Sequence[int]):
        """Longest cached block-aligned prefix of `tokens`.

        Returns (n_tokens_hit, blocks) — blocks in order, each covering
        [i*bs, (i+1)*bs).
        """
        hit: List[_Block] = []
        toks = tuple(tokens)
        for i, (key, _blk) in enumerate(self._chain_keys(toks)):
            ent = self._blocks.get(key)
            if ent is None or ent.prefix != toks[: (i + 1) * self.bs]:
                break
            self._blocks.move_to_end(key)
            hit.append(ent)
        n = len(hit) * self.bs
        if n:
            self.hits += 1
            self.tokens_reused += n
        else:
            self.misses += 1
        return n, hit

    # ----------------------------------------------------------- insert
    def insert(self, tokens: Sequence[int], cache, row: int = 0,
               upto: int = None) -> int:
        """Store the block-aligned prefix of `tokens` from live KVCache
        row `row` (cache.k/v: [L, B, Hk, T, D], positions [0, len(tokens))
        already prefilled). Returns the number of NEW blocks stored."""
        toks = tuple(tokens)
        if upto is not None:
            toks = toks[: int(upto)]
        new = 0
        for i, (key, _blk) in enumerate(self._chain_keys(toks)):
            ent = self._blocks.get(key)
            if ent is not None and ent.prefix == toks[: (i + 1) * self.bs]:
                self._blocks.move_to_end(key)
                continue
            sl = slice(i * self.bs, (i + 1) * self.bs)
            kb = cache.k[:, row, :, sl].clone()
            vb = cache.v[:, row, :, sl].clone()
            if ent is not None:  # hash collision: latest wins
                self._bytes -= (ent.k.numel() + ent.v.numel()) * 2
            self._blocks[key] = _Block(toks[: (i + 1) * self.bs], kb, vb)
            self._blocks.move_to_end(key)
            self._bytes += (kb.numel() + vb.numel()) * 2
            new += 1
        while self._bytes > self.budget and len(self._blocks) > 1:
            _, old = self._blocks.popitem(last=False)
            self._bytes -= (old.k.numel() + old.v.numel()) * 2
        return new

    # ------------------------------------------------------------- seed
    def seed(self, cache, blocks: List[_Block]) -> None:
        """Copy hit blocks into ALL rows of a live KVCache (positions
        [0, len(blocks)*bs)). Rows beyond the real batch are pad rows
        replaying row 0's prompt, so broadcasting is correct."""
        for i, ent in enumerate(blocks):
            sl = slice(i * self.bs, (i + 1) * self.bs)
            cache.k[:, :, :, sl] = ent.k.unsqueeze(1)
            cache.v[:, :, :, sl] = ent.v.unsqueeze(1)

    def seed_row(self, cache, blocks: List[_Block], row: int) -> None:
        """Copy hit blocks into ONE row (continuous-batching slots)."""
        for i, ent in enumerate(blocks):
            sl = slice(i * self.bs, (i + 1) * self.bs)
            cache.k[:, row, :, sl] = ent.k
            cache.v[:, row, :, sl] = ent.v

    def stats(self) -> dict:
        return {"blocks": len(self._blocks), "bytes": self._bytes,
                "hits": self.hits, "misses": self.misses,
                "tokens_reused": self.tokens_reused}


def prefix_cache_from_env() -> "PrefixKVCache | None":
    """Engine-side factory: ANTRAY_PREFIX_CACHE=0 disables; block size /
    budget via ANTRAY_PREFIX_BLOCK (64) / ANTRAY_PREFIX_CACHE_MB (512)."""
    if os.environ.get("ANTRAY_PREFIX_CACHE", "1") == "0":
        return None
    return PrefixKVCache(
        block_size=int(os.environ.get("ANTRAY_PREFIX_BLOCK", "64")),
        budget_mb=float(os.environ.get("ANTRAY_PREFIX_CACHE_MB", "512")))
