"""The paged-KV entry points must be linked into _hip_ops (a partial
relink that drops attention_decode.o / rope.o would otherwise only fail
on the GPU box)."""
import pytest


def test_hip_ops_has_paged_decode():
    pytest.importorskip("torch")

    import ant_ray_amd._hip_ops as m

    for fn in ("attn_decode_paged", "decode_step_attn_paged",
               "attn_decode", "decode_step_attn"):
        assert hasattr(m, fn), f"_hip_ops is missing {fn}"
