"""Paged KV cache on the MI355X: the paged flash-decode kernel and the
paged device-pos decode step (csrc/kernels/attention_decode.hip,
rope.hip) against the fp32 reference and the contiguous kernels, and the
paged continuous engine end to end."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ant_ray_amd import ops
    from ant_ray_amd.ops import reference as ref

    DEV = "cuda:0"


def _close(a, b, what, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), atol=atol,
                               rtol=rtol, msg=what)


def _scatter(k, v, P, seed=0):
    """Contiguous [B,Hk,T,D] K/V -> shuffled pages of a pool with page 0
    left as a (garbage-filled) trash page. Returns (kp, vp, table)."""
    B, Hk, T, D = k.shape
    W = T // P
    g = torch.Generator().manual_seed(seed)
    table = (torch.randperm(B * W, generator=g) + 1).view(B, W)
    kp = torch.randn(B * W + 1, Hk, P, D, dtype=k.dtype, device=k.device)
    vp = torch.randn_like(kp)
    kb = k.view(B, Hk, W, P, D).permute(0, 2, 1, 3, 4)
    vb = v.view(B, Hk, W, P, D).permute(0, 2, 1, 3, 4)
    t = table.to(k.device)
    kp[t.reshape(-1)] = kb.reshape(B * W, Hk, P, D)
    vp[t.reshape(-1)] = vb.reshape(B * W, Hk, P, D)
    return kp, vp, t.to(torch.int32).contiguous()


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(4321)


class TestAttentionDecodePaged:
    @pytest.mark.parametrize("case", [
        # (B, Hq, Hk, T, P, lens)
        ("uniform", 4, 32, 8, 1024, 64, [777] * 4),
        ("ragged", 5, 8, 4, 512, 16, [3, 100, 512, 77, 256]),
        ("multichunk", 1, 32, 8, 4096, 64, [4096]),
        ("non_page_multiple", 3, 16, 8, 640, 32, [639, 33, 1]),
        ("gq1", 2, 8, 8, 256, 16, [200, 17]),
        ("gq2", 2, 8, 4, 256, 32, [256, 130]),
        ("gq8", 2, 64, 8, 512, 64, [500, 65]),
    ], ids=lambda c: c[0])
    def test_vs_reference(self, case):
        _, B, Hq, Hk, T, P, lens = case
        D = 128
        q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=DEV)
        k = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV)
        v = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV)
        kp, vp, table = _scatter(k, v, P)
        ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
        o = ops.attention_decode_paged(q, kp, vp, table, ln)
        o_ref = ref.attention_decode_ref(q, k, v, lens=ln)
        _close(o, o_ref, f"paged decode {case[0]}")
        # the CPU reference over the same pages agrees too
        _close(ref.attention_decode_paged_ref(q, kp, vp, table, ln), o_ref,
               "paged reference", atol=1e-2, rtol=1e-2)

    def test_spiked_key(self):
        # forces the defer-max rescale branch inside a late page
        B, Hq, Hk, T, P, D = 2, 4, 2, 320, 32, 128
        q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=DEV)
        k = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV) * 0.1
        v = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV)
        k[:, :, 237] = q[:, ::2, :] * 3.0
        kp, vp, table = _scatter(k, v, P)
        ln = torch.tensor([300, 300], dtype=torch.int32, device=DEV)
        o = ops.attention_decode_paged(q, kp, vp, table, ln)
        _close(o, ref.attention_decode_ref(q, k, v, lens=ln), "spiked")

    def test_paged_step_vs_contiguous_step(self):
        B, Hq, Hk, T, P, D = 4, 32, 8, 512, 64, 128
        cos, sin = ops.rope_tables(D, T, device=DEV)
        ck = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV)
        cv = torch.randn(B, Hk, T, D, dtype=torch.bfloat16, device=DEV)
        kp, vp, table = _scatter(ck, cv, P, seed=2)
        lens = torch.tensor([1, 65, 300, 512], dtype=torch.int32,
                            device=DEV)
        qkv = torch.randn(B, 1, (Hq + 2 * Hk) * D, dtype=torch.bfloat16,
                          device=DEV)
        o_c = ops.decode_step_attn(qkv.clone(), ck, cv, lens, cos, sin, Hq,
                                   Hk)
        o_p = ops.decode_step_attn_paged(qkv.clone(), kp, vp, table, lens,
                                         cos, sin, Hq, Hk)
        _close(o_p, o_c, "paged step vs contiguous step")
        # the new K/V rows landed at the right page slots
        _close(ref.gather_pages(kp, table), ck, "pool after write",
               atol=0, rtol=0)
        _close(ref.gather_pages(vp, table), cv, "pool after write v",
               atol=0, rtol=0)


class TestPagedEngine:
    def test_paged_engine_graph_and_tokens(self, monkeypatch):
        """The paged continuous engine captures its step graph and its
        leading tokens agree with the contiguous engine's."""
        from ant_ray_amd.llm.continuous import ContinuousLLMEngine

        monkeypatch.setenv("ANTRAY_PREFIX_CACHE", "0")
        paged = ContinuousLLMEngine("llama-tiny-d128", slots=4, max_seq=256,
                                    device=DEV, kv_cache="paged",
                                    block_size=16)
        contig = ContinuousLLMEngine("llama-tiny-d128", slots=4,
                                     max_seq=256, device=DEV)
        torch.manual_seed(9)
        prompts = [torch.randint(0, 1024, (n,)).tolist()
                   for n in (9, 13, 7, 21, 5, 40)]
        outs = {}
        for name, eng in (("paged", paged), ("contig", contig)):
            futs = [eng.submit(p, 12) for p in prompts]
            eng.run_until_idle()
            assert eng.dec.graph is not None, f"{name}: no step graph"
            outs[name] = [f.result(timeout=0) for f in futs]
        st = paged.stats()
        assert st["active"] == 0 and st["pages_used"] == 0
        assert paged.dec.lens.tolist() == [1, 1, 1, 1]
        for p, a, b in zip(prompts, outs["paged"], outs["contig"]):
            assert len(a) == 12
            # same weights (seed 0); the kernels differ only in chunk
            # boundaries (16-aligned in the paged split), which can
            # tie-flip late tokens of a random-init model in bf16
            assert a[:4] == b[:4], (p, a, b)

    def test_paged_prefix_hit_logits(self, monkeypatch):
        """A prefix-hit request (shared pages gathered for chunked
        prefill) gives the same next-token logits as an uncached run."""
        from ant_ray_amd.llm.continuous import ContinuousLLMEngine

        monkeypatch.setenv("ANTRAY_PREFIX_CACHE", "1")
        eng = ContinuousLLMEngine("llama-tiny-d128", slots=2, max_seq=256,
                                  device=DEV, kv_cache="paged",
                                  block_size=16)
        torch.manual_seed(5)
        sysp = torch.randint(0, 1024, (48,)).tolist()
        p1 = sysp + torch.randint(0, 1024, (9,)).tolist()
        p2 = sysp + torch.randint(0, 1024, (9,)).tolist()
        eng.submit(p1, 8)
        eng.run_until_idle()
        assert eng.stats()["pages_cached"] == 3
        m = eng.model
        bm = eng.blocks
        # replay p2's admission by hand to read its prefill logits
        hit = bm.lookup(p2[:-1])
        assert len(hit) == 3
        pages = hit + bm.alloc(2)
        toks = torch.tensor([p2], dtype=torch.long, device=DEV)
        with torch.no_grad():
            split = m.forward(toks[:, 48:], cache=eng.dec.cache.seq_view(
                pages), pos=48)
            full = m.forward(toks, cache=eng.dec.cache.seq_view(
                bm.alloc(5)), pos=0)
        torch.testing.assert_close(full.float(), split.float(), rtol=5e-2,
                                   atol=5e-2)
