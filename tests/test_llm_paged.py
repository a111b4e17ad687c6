"""Paged KV cache for the continuous engine (llm/kv_blocks.py,
llm/continuous.py kv_cache="paged", models/llama.py PagedKVCache).

On CPU every op runs the exact fp32 reference (the paged decode step
gathers pages and calls the contiguous reference), so paged outputs must
equal per-request model.generate() exactly.
"""
import random

import pytest
import torch

from ant_ray_amd.llm.continuous import ContinuousLLMEngine
from ant_ray_amd.llm.kv_blocks import BlockManager, plan_admission
from ant_ray_amd.ops import reference as ref

BS = 16


def _ref_tokens(model, prompt, n):
    toks = torch.tensor([prompt], dtype=torch.long)
    return model.generate(toks, n)[0, len(prompt):].tolist()


def _engine(slots=2, max_seq=128, **kw):
    return ContinuousLLMEngine("llama-tiny", slots=slots, max_seq=max_seq,
                               device="cpu", kv_cache="paged",
                               block_size=BS, **kw)


@pytest.fixture()
def no_share(monkeypatch):
    monkeypatch.setenv("ANTRAY_PREFIX_CACHE", "0")


def test_paged_matches_generate_with_queueing(no_share):
    eng = _engine(slots=2)
    prompts = [[5, 6, 7], [9, 8, 7, 6, 5] * 5, [11, 12], [3, 3, 3, 3]]
    news = [6, 4, 5, 3]
    futs = [eng.submit(p, n) for p, n in zip(prompts, news)]
    eng.run_until_idle()
    for p, n, f in zip(prompts, news, futs):
        assert f.result(timeout=0) == _ref_tokens(eng.model, p, n), (p, n)
    st = eng.stats()
    assert st["active"] == 0 and st["queued"] == 0
    assert st["steps"] <= sum(news)


def test_paged_mid_run_admission(no_share):
    eng = _engine(slots=4)
    f1 = eng.submit([42, 17, 8, 100], 20)
    for _ in range(4):
        eng.pump()
    f2 = eng.submit([7, 7, 7], 5)
    eng.run_until_idle()
    assert f1.result(timeout=0) == _ref_tokens(eng.model, [42, 17, 8, 100],
                                               20)
    assert f2.result(timeout=0) == _ref_tokens(eng.model, [7, 7, 7], 5)


def test_paged_slot_reuse_isolation(no_share):
    eng = _engine(slots=1)
    p1 = list(range(100, 130))
    f1 = eng.submit(p1, 8)
    f2 = eng.submit([55, 44], 6)  # reuses slot 0 (and freed pages)
    eng.run_until_idle()
    assert f1.result(timeout=0) == _ref_tokens(eng.model, p1, 8)
    assert f2.result(timeout=0) == _ref_tokens(eng.model, [55, 44], 6)


def test_paged_small_pool_waits_then_completes(no_share):
    # 5 usable pages of 16 tokens; each request needs 2 pages, so only
    # two of four slots can run at once — the rest wait, FIFO
    from ant_ray_amd.models.llama import PagedKVCache

    eng0 = _engine(slots=4)
    pb = PagedKVCache.page_bytes(eng0.model.cfg, BS)
    eng = _engine(slots=4, kv_pool_mb=6 * pb / (1 << 20))
    assert eng.stats()["pages_total"] == 5
    rng = random.Random(4)
    prompts = [[rng.randrange(1024) for _ in range(10 + i)]
               for i in range(4)]
    futs = [eng.submit(p, 8) for p in prompts]
    eng.pump()
    st = eng.stats()
    assert st["active"] == 2 and st["queued"] == 2
    assert st["pages_free"] == 1
    eng.run_until_idle()
    for p, f in zip(prompts, futs):
        assert f.result(timeout=0) == _ref_tokens(eng.model, p, 8)
    assert eng.stats()["pages_peak_used"] <= 5


def test_paged_request_larger_than_pool_rejected(no_share):
    from ant_ray_amd.models.llama import PagedKVCache

    eng0 = _engine()
    pb = PagedKVCache.page_bytes(eng0.model.cfg, BS)
    eng = _engine(kv_pool_mb=4 * pb / (1 << 20))  # 3 usable pages
    with pytest.raises(ValueError):
        eng.submit(list(range(40)), 20)  # 60 tokens -> 4 pages
    eng.submit(list(range(30)), 10).result  # 40 tokens -> 3 pages: fits


def test_paged_shared_prefix_by_reference(monkeypatch):
    monkeypatch.setenv("ANTRAY_PREFIX_CACHE", "1")
    eng = _engine(slots=2)
    rng = random.Random(3)
    sysp = [rng.randrange(256) for _ in range(3 * BS)]
    p0 = sysp + [1, 2, 3]
    f0 = eng.submit(p0, 5)  # cold: writes + registers 3 prompt pages
    eng.run_until_idle()
    assert eng.stats()["pages_cached"] == 3
    pa = sysp + [rng.randrange(256) for _ in range(4)]
    pb = sysp + [rng.randrange(256) for _ in range(5)]
    fa = eng.submit(pa, 5)
    fb = eng.submit(pb, 5)
    eng.pump()
    st = eng.stats()
    assert st["active"] == 2
    assert st["pages_shared"] == 3          # both rows map the same pages
    # each request reserves ceil((len+5)/16) = 4 pages, 3 of them shared:
    # 3 shared + 1 private each, no copy
    assert st["pages_used"] == 3 + 1 + 1
    eng.run_until_idle()
    for p, f in ((p0, f0), (pa, fa), (pb, fb)):
        assert f.result(timeout=0) == _ref_tokens(eng.model, p, 5)
    assert eng.stats()["prefix_pages_hit"] == 6


def test_paged_stop_token_frees_pages_early(no_share):
    eng = _engine(slots=2)
    p = [21, 22, 23, 24]
    ref_toks = _ref_tokens(eng.model, p, 40)
    stop = ref_toks[3]
    k = ref_toks.index(stop) + 1
    f = eng.submit(p, 40, stop_token_ids=[stop])
    eng.pump()
    assert eng.stats()["pages_used"] == 3  # ceil(44/16)
    for _ in range(k):
        eng.pump()
    assert f.done() and f.result(timeout=0) == ref_toks[:k]
    assert eng.stats()["pages_used"] == 0


def test_paged_pages_free_returns_after_idle(monkeypatch):
    monkeypatch.setenv("ANTRAY_PREFIX_CACHE", "1")
    eng = _engine(slots=3)
    start = eng.stats()["pages_free"]
    rng = random.Random(9)
    futs = [eng.submit([rng.randrange(1024) for _ in range(rng.randrange(
        5, 40))], rng.randrange(2, 12)) for _ in range(7)]
    eng.run_until_idle()
    assert all(f.done() for f in futs)
    st = eng.stats()
    assert st["pages_free"] == start and st["pages_used"] == 0


def test_idle_slots_stay_on_trash_page(no_share):
    eng = _engine(slots=3)
    f = eng.submit([1, 2, 3, 4, 5], 10)
    eng.run_until_idle()
    assert f.done()
    assert eng.dec.lens.tolist() == [1, 1, 1]
    assert eng.dec.cache.block_table.abs().sum().item() == 0


# ------------------------------------------------------- block manager
def test_block_manager_tail_first_eviction():
    bm = BlockManager(n_pages=7, block_size=4)  # 6 usable
    chain = list(range(100, 116))               # 4 full blocks
    pages = bm.alloc(4)
    assert bm.register(chain, pages) == 4
    bm.release(pages)
    assert bm.cached() == 4 and bm.available() == 6
    # touch only the head, making it most recent; then force eviction
    # of 3 pages: a middle-first LRU would drop the older tail blocks
    # too, but must never leave a page whose parent is gone
    hit = bm.lookup(chain[:5])
    assert hit == pages[:1]
    bm.release(hit)
    got = bm.alloc(5)
    assert len(got) == 5
    assert bm.unreachable_cached() == 0
    assert bm.cached() == 1
    # what remains cached is a reachable prefix of the chain
    assert bm.lookup(chain + [0]) == pages[:1]


def test_block_manager_eviction_keeps_reachability_randomized():
    rng = random.Random(0)
    bm = BlockManager(n_pages=33, block_size=4)
    held = []
    for _ in range(400):
        if held and (rng.random() < 0.5 or bm.available() < 6):
            bm.release(held.pop(rng.randrange(len(held))))
            continue
        base = rng.randrange(3)
        toks = [base] * 8 + [rng.randrange(4) for _ in range(rng.randrange(
            1, 12))]
        plan = plan_admission(bm, toks, 3, share=True)
        if plan is None:
            continue
        pages, _ = plan
        bm.register(toks, pages)
        held.append(pages)
        assert bm.unreachable_cached() == 0
    for p in held:
        bm.release(p)
    assert bm.used() == 0 and bm.unreachable_cached() == 0


def test_block_manager_hash_collision_is_not_a_hit(monkeypatch):
    bm = BlockManager(n_pages=5, block_size=2)
    pages = bm.alloc(2)
    bm.register([1, 2, 3, 4], pages)
    # forge the index key of a different chain onto page 0
    key = hash((0, (9, 9)))
    bm._index[key] = pages[0]
    assert bm.lookup([9, 9, 5]) == []


# ------------------------------------------------------ op references
@pytest.mark.parametrize("gq", [1, 2, 4])
def test_paged_reference_equals_contiguous(gq):
    torch.manual_seed(0)
    B, Hk, D, P, W = 3, 2, 32, 16, 5
    Hq = Hk * gq
    T = W * P
    q = torch.randn(B, Hq, D, dtype=torch.bfloat16)
    k = torch.randn(B, Hk, T, D, dtype=torch.bfloat16)
    v = torch.randn(B, Hk, T, D, dtype=torch.bfloat16)
    lens = torch.tensor([1, 37, T], dtype=torch.int32)
    n_pages = B * W + 1
    perm = torch.randperm(n_pages - 1)[: B * W] + 1     # shuffled, no 0
    table = perm.view(B, W).to(torch.int32)
    kp = torch.zeros(n_pages, Hk, P, D, dtype=torch.bfloat16)
    vp = torch.zeros_like(kp)
    for b in range(B):
        for w in range(W):
            kp[table[b, w]] = k[b, :, w * P : (w + 1) * P]
            vp[table[b, w]] = v[b, :, w * P : (w + 1) * P]
    o_c = ref.attention_decode_ref(q, k, v, lens=lens)
    o_p = ref.attention_decode_paged_ref(q, kp, vp, table, lens)
    assert torch.equal(o_c, o_p)


def test_paged_decode_step_reference_equals_contiguous():
    from ant_ray_amd import ops

    torch.manual_seed(1)
    B, Hq, Hk, D, P, W = 2, 4, 2, 64, 16, 4
    T = W * P
    cos, sin = ops.rope_tables(D, T)
    ck = torch.randn(B, Hk, T, D, dtype=torch.bfloat16)
    cv = torch.randn(B, Hk, T, D, dtype=torch.bfloat16)
    table = (torch.randperm(B * W) + 1).view(B, W).to(torch.int32)
    kp = torch.zeros(B * W + 1, Hk, P, D, dtype=torch.bfloat16)
    vp = torch.zeros_like(kp)
    for b in range(B):
        for w in range(W):
            kp[table[b, w]] = ck[b, :, w * P : (w + 1) * P]
            vp[table[b, w]] = cv[b, :, w * P : (w + 1) * P]
    lens = torch.tensor([20, 64], dtype=torch.int32)
    qkv = torch.randn(B, 1, (Hq + 2 * Hk) * D, dtype=torch.bfloat16)
    o_c = ops.decode_step_attn(qkv, ck, cv, lens, cos, sin, Hq, Hk)
    o_p = ops.decode_step_attn_paged(qkv, kp, vp, table, lens, cos, sin,
                                     Hq, Hk)
    assert torch.equal(o_c, o_p)
    assert torch.equal(ref.gather_pages(kp, table), ck)


# ------------------------------------------------------------- serve
@pytest.fixture()
def ray_cpu():
    import ant_ray_amd as ray

    if ray.is_initialized():
        ray.shutdown()
    ray.init(num_cpus=4)
    yield ray
    ray.shutdown()


def test_serve_paged_kv_continuous(ray_cpu):
    from ant_ray_amd import serve
    from ant_ray_amd.llm import LLMConfig, build_llm_deployment
    from ant_ray_amd.models import build_model

    app = build_llm_deployment(LLMConfig(
        model_loading_config={"model_id": "llama-tiny"},
        engine_kwargs={"max_model_len": 64, "max_num_seqs": 4,
                       "tensor_parallel_size": 0,
                       "continuous_batching": True, "paged_kv": True,
                       "block_size": 16, "kv_cache_memory_mb": 1},
        deployment_config={"num_replicas": 1},
    ))
    h = serve.run(app, name="llm-pg", route_prefix="/llm-pg")
    rng = random.Random(2)
    prompts = [[rng.randrange(1024) for _ in range(rng.randrange(4, 16))]
               for _ in range(6)]
    outs = [r.result(timeout_s=300)["token_ids"] for r in
            [h.remote({"prompt_ids": p, "max_new_tokens": 6})
             for p in prompts]]
    serve.shutdown()
    torch.manual_seed(0)
    m = build_model("llama-tiny", device="cpu", seq_len=64)
    m.eval()
    for p, o in zip(prompts, outs):
        assert o == _ref_tokens(m, p, 6)


def test_paged_kv_requires_continuous():
    from ant_ray_amd.llm import LLMConfig, build_llm_deployment

    with pytest.raises(ValueError, match="continuous"):
        build_llm_deployment(LLMConfig(
            model_loading_config={"model_id": "llama-tiny"},
            engine_kwargs={"max_model_len": 64, "tensor_parallel_size": 0,
                           "paged_kv": True},
        ))


def test_paged_rejects_bad_block_size():
    with pytest.raises(ValueError):
        ContinuousLLMEngine("llama-tiny", slots=1, max_seq=64,
                            device="cpu", kv_cache="paged", block_size=8)
