"""lora_group_forward(x, mods, rope=...) on the CPU: the modules one by one,
then ops.rope on the flagged outputs — and LlamaAttention, which now asks the
group for rotated q and k, still computes the composition it did before."""

import pytest
import torch

from relora_amd import ops
from relora_amd.models.config import LlamaConfig
from relora_amd.models.llama import LlamaAttention
from relora_amd.relora import ReLoRaLinear, lora_group_forward


def make_modules(K, Ns, r, dtype=torch.float32):
    torch.manual_seed(31)
    mods = []
    for N in Ns:
        m = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, bias=False)
        with torch.no_grad():
            m.lora_B.weight.normal_(std=0.05)
        mods.append(m.to(dtype).eval())
    return mods


def heads(y, hd):
    return y.view(y.shape[0], y.shape[1], -1, hd).transpose(1, 2)


@pytest.mark.parametrize("hd,Ns,flags", [
    (16, (64, 64, 64), (True, True, False)),
    (16, (64, 32, 32), (True, True, False)),     # GQA
    (64, (128, 64), (True, False)),              # a lone rotary sibling
    (24, (48, 48, 48), (True, True, False)),     # no kernel would take this head_dim
])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_arg_equals_modules_then_rope(hd, Ns, flags, dtype):
    B, S, K = 2, 12, 32
    mods = make_modules(K, Ns, 8, dtype)
    x = torch.randn(B, S, K).to(dtype)
    cos, sin = ops.build_rope_cache(hd, 20)
    got = lora_group_forward(x, mods, rope=(cos, sin, flags, hd))
    want = [m(x) for m in mods]
    assert len(got) == len(want)
    for g, f in enumerate(flags):
        assert got[g].shape == want[g].shape
        if f:
            w, _ = ops.rope(heads(want[g], hd), heads(want[g], hd), cos, sin)
            assert torch.equal(heads(got[g], hd), w), g
            assert not torch.equal(got[g], want[g])
        else:
            assert torch.equal(got[g], want[g]), g


def test_rope_none_is_unchanged():
    mods = make_modules(32, (64, 64), 8)
    x = torch.randn(2, 12, 32)
    for a, b in zip(lora_group_forward(x, mods), [m(x) for m in mods]):
        assert torch.equal(a, b)
    for a, b in zip(lora_group_forward(x, mods, rope=None), [m(x) for m in mods]):
        assert torch.equal(a, b)


def test_rope_arg_checks_shapes():
    mods = make_modules(32, (64, 64), 8)
    cos, sin = ops.build_rope_cache(16, 20)
    with pytest.raises(ValueError):  # one flag per module
        lora_group_forward(torch.randn(2, 12, 32), mods, rope=(cos, sin, (True,), 16))
    with pytest.raises(ValueError):  # [B, S, K] only
        lora_group_forward(torch.randn(24, 32), mods, rope=(cos, sin, (True, True), 16))


def parent_attention(attn, x, position_ids=None, past=None):
    """LlamaAttention.forward as it was: project, view as heads, ops.rope."""
    B, S, _ = x.shape
    q, k, v = [m(x) for m in (attn.q_proj, attn.k_proj, attn.v_proj)]
    q = q.view(B, S, attn.num_heads, attn.head_dim).transpose(1, 2)
    k = k.view(B, S, attn.num_key_value_heads, attn.head_dim).transpose(1, 2)
    v = v.view(B, S, attn.num_key_value_heads, attn.head_dim).transpose(1, 2)
    kv_len = S + (past[0].shape[-2] if past is not None else 0)
    cos, sin = attn.rotary_emb(v, seq_len=kv_len)
    if past is not None and position_ids is None:
        position_ids = torch.arange(kv_len - S, kv_len).unsqueeze(0)
    q, k = ops.rope(q, k, cos, sin, position_ids=position_ids)
    if past is not None:
        k = torch.cat([past[0], k], dim=2)
        v = torch.cat([past[1], v], dim=2)
    o = ops.flash_attention(q, k, v, causal=S > 1)
    return attn.o_proj(o.transpose(1, 2).reshape(B, S, attn.hidden_size)), (k, v)


@pytest.mark.parametrize("nkv", [4, 2])
def test_llama_attention_unchanged(nkv):
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=176,
                      num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=nkv,
                      max_position_embeddings=32)
    attn = LlamaAttention(cfg).eval()
    x = torch.randn(2, 12, 64)
    with torch.no_grad():
        # no cache: q and k come rotated out of the projection group
        got, _ = attn(x)
        want, _ = parent_attention(attn, x)
        assert torch.equal(got, want)
        # explicit position_ids: the two separate calls, as before
        pos = torch.arange(12).unsqueeze(0).expand(2, 12)
        got, _ = attn(x, position_ids=pos)
        want, _ = parent_attention(attn, x, position_ids=pos)
        assert torch.equal(got, want)
        # prefill 8 tokens, then 4 more against the cache
        got0, present = attn(x[:, :8], use_cache=True)
        want0, wpast = parent_attention(attn, x[:, :8])
        assert torch.equal(got0, want0)
        assert torch.equal(present[0], wpast[0]) and torch.equal(present[1], wpast[1])
        got1, _ = attn(x[:, 8:], past_key_value=present)
        want1, _ = parent_attention(attn, x[:, 8:], past=wpast)
        assert torch.equal(got1, want1)
