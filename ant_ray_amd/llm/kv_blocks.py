"""Page allocator + prefix index for the paged KV cache.

Role parity: vLLM's block manager with automatic prefix caching (the
reference delegates serving to vLLM, reference python/ray/llm/_internal/
serve/engines/vllm/vllm_engine.py:1). Host-side bookkeeping only; the
pages themselves are rows of models/llama.py PagedKVCache pools (layout
documented at the top of csrc/kernels/attention_decode.hip).

  * Page 0 is the TRASH page: every unused block-table entry points at
    it, so an idle decode slot that keeps stepping writes there and never
    into a live page. It is never allocated.
  * Pages carry refcounts. A page is FREE (on the free list), HELD (ref
    > 0) or CACHED-IDLE (ref == 0 but still indexed for prefix reuse).
    Cached-idle pages count as available: alloc() evicts them on demand.
  * Prefix index: the same chain key as llm/prefix_cache.py (rolling
    hash over the block chain) plus an exact check of the block's tokens
    and its parent page, so a hit is exact. A full prompt page is
    registered once its K/V is written. Sharing is safe because lookups
    never cover a request's last prompt token, so every shared page lies
    wholly before the first position the request writes.
  * Eviction is LRU over cached-idle pages that have no cached child:
    chain TAILS go first, so a cached chain never loses a middle page and
    strands the pages after it.
"""
from __future__ import annotations

import heapq
import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

TRASH_PAGE = 0


@dataclass
class _Entry:
    key: int
    tokens: tuple          # this page's block tokens
    parent: int            # parent page id (-1 for a chain head)
    children: int = 0      # cached pages whose parent is this page
    last_use: int = 0


class BlockManager:
    def __init__(self, n_pages: int, block_size: int):
        if n_pages < 2:
            raise ValueError("paged KV pool needs at least 2 pages "
                             "(page 0 is the trash page)")
        self.n_pages = int(n_pages)
        self.bs = int(block_size)
        self._free: List[int] = list(range(self.n_pages - 1, 0, -1))
        self._ref = [0] * self.n_pages
        self._index: Dict[int, int] = {}          # chain key -> page
        self._entry: Dict[int, _Entry] = {}       # page -> index entry
        self._idle_cached = 0                     # cached pages, ref == 0
        self._heap: List[Tuple[int, int]] = []    # (last_use, page)
        self._clock = itertools.count(1)
        self.peak_used = 0
        self.hit_pages = 0

    # ------------------------------------------------------------ counts
    @property
    def total(self) -> int:
        return self.n_pages - 1

    def available(self) -> int:
        """Pages alloc() can hand out now (free + evictable cached)."""
        return len(self._free) + self._idle_cached

    def used(self) -> int:
        return self.total - self.available()

    def shared(self) -> int:
        return sum(1 for r in self._ref if r > 1)

    def pages_needed(self, n_tokens: int) -> int:
        return -(-int(n_tokens) // self.bs)

    # -------------------------------------------------------- refcounts
    def _incref(self, page: int) -> None:
        if self._ref[page] == 0 and page in self._entry:
            self._idle_cached -= 1
        self._ref[page] += 1

    def _decref(self, page: int) -> None:
        self._ref[page] -= 1
        if self._ref[page] > 0:
            return
        ent = self._entry.get(page)
        if ent is None:
            self._free.append(page)
            return
        self._idle_cached += 1
        ent.last_use = next(self._clock)
        if ent.children == 0:
            heapq.heappush(self._heap, (ent.last_use, page))

    def _evictable(self, page: int, stamp: int) -> bool:
        ent = self._entry.get(page)
        return (ent is not None and self._ref[page] == 0
                and ent.children == 0 and ent.last_use == stamp)

    def _evict_one(self) -> int:
        while self._heap:
            stamp, page = heapq.heappop(self._heap)
            if not self._evictable(page, stamp):
                continue  # stale heap record
            ent = self._entry.pop(page)
            del self._index[ent.key]
            self._idle_cached -= 1
            if ent.parent >= 0:
                par = self._entry[ent.parent]
                par.children -= 1
                if par.children == 0 and self._ref[ent.parent] == 0:
                    # the parent is now a tail: it becomes evictable with
                    # its own LRU stamp
                    heapq.heappush(self._heap, (par.last_use, ent.parent))
            return page
        raise RuntimeError("paged KV pool exhausted")

    # ------------------------------------------------------------ alloc
    def alloc(self, n: int) -> List[int]:
        """n fresh pages (ref 1), evicting cached-idle tails as needed.
        Callers check available() first."""
        if n > self.available():
            raise RuntimeError(f"paged KV pool: need {n} pages, "
                               f"{self.available()} available")
        out = []
        for _ in range(n):
            page = self._free.pop() if self._free else self._evict_one()
            self._ref[page] = 1
            out.append(page)
        self.peak_used = max(self.peak_used, self.used())
        return out

    def release(self, pages: Sequence[int]) -> None:
        for p in pages:
            self._decref(p)

    # ----------------------------------------------------- prefix index
    def _chain(self, tokens: Sequence[int]):
        chain = 0
        for i in range(len(tokens) // self.bs):
            blk = tuple(tokens[i * self.bs : (i + 1) * self.bs])
            chain = hash((chain, blk))
            yield chain, blk

    def lookup(self, tokens: Sequence[int]) -> List[int]:
        """Longest cached page chain covering full blocks of `tokens`.
        Returned pages are referenced (ref += 1) for the caller; give
        them back with release()."""
        hit: List[int] = []
        parent = -1
        for key, blk in self._chain(tokens):
            page = self._index.get(key)
            if page is None:
                break
            ent = self._entry[page]
            if ent.tokens != blk or ent.parent != parent:
                break  # hash collision: not this chain
            hit.append(page)
            parent = page
        for p in hit:
            self._incref(p)
        self.hit_pages += len(hit)
        return hit

    def register(self, tokens: Sequence[int], pages: Sequence[int]) -> int:
        """Index the full blocks of `tokens` (already written into
        `pages`, in order). Blocks already indexed keep their page.
        Returns the number of newly indexed pages."""
        new = 0
        parent = -1
        for i, (key, blk) in enumerate(self._chain(tokens)):
            page = self._index.get(key)
            if page is not None:
                ent = self._entry[page]
                if ent.tokens == blk and ent.parent == parent:
                    parent = page
                    continue
                break  # collision with a different chain: stop indexing
            page = pages[i]
            if page in self._entry:
                break
            self._index[key] = page
            self._entry[page] = _Entry(key, blk, parent,
                                       last_use=next(self._clock))
            if parent >= 0:
                self._entry[parent].children += 1
            parent = page
            new += 1
        return new

    # ------------------------------------------------------------ debug
    def cached(self) -> int:
        return len(self._entry)

    def unreachable_cached(self) -> int:
        """Indexed pages whose chain no longer leads back to a head (must
        always be 0: tail-first eviction never strands a page)."""
        return sum(1 for e in self._entry.values()
                   if e.parent >= 0 and e.parent not in self._entry)

    def stats(self) -> dict:
        return {"pages_total": self.total, "pages_free": self.available(),
                "pages_used": self.used(), "pages_cached": self.cached(),
                "pages_shared": self.shared(),
                "pages_peak_used": self.peak_used,
                "prefix_pages_hit": self.hit_pages}


def plan_admission(bm: BlockManager, prompt: Sequence[int], max_new: int,
                   share: bool) -> Optional[Tuple[List[int], int]]:
    """Reserve every page a request can touch: ceil((len(prompt) +
    max_new) / P) minus the shared prefix pages. Returns (pages, n_hit)
    with pages[:n_hit] shared, or None (nothing held) when the pool is
    short right now."""
    need = bm.pages_needed(len(prompt) + max_new)
    hit = bm.lookup(prompt[: len(prompt) - 1]) if share else []
    if need - len(hit) > bm.available():
        bm.release(hit)
        if share:
            bm.hit_pages -= len(hit)
        return None
    return hit + bm.alloc(need - len(hit)), len(hit)
