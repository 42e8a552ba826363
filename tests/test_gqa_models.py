"""Grouped-query attention above the kernels, on the CPU: config, the SDPA
path of `ops.flash_attention`, Hugging Face checkpoint interchange in both
directions, `.generate()`, ReLoRA merge + round trip, the memory estimate,
and the conditioning of the inputs tests/test_gpu_attention_gqa.py uses."""

import glob
import json
import os

import pytest
import torch
import torch.nn.functional as F

import attn_variant_worker as aw
import gqa_common as gc
from relora_amd import ops
from relora_amd.models.config import LlamaConfig, load_model_config
from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.utils.checkpoint import save_pretrained_compat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "reference_parity")


def tiny_gqa_config(**kw):
    d = dict(vocab_size=128, hidden_size=64, intermediate_size=96,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             max_position_embeddings=64, bos_token_id=0, eos_token_id=1)
    d.update(kw)
    return LlamaConfig(**d)


# -- config -------------------------------------------------------------------

def test_config_default_roundtrip_and_divisor(tmp_path):
    assert LlamaConfig(num_attention_heads=8).num_key_value_heads == 8
    cfg = tiny_gqa_config()
    assert cfg.num_key_value_heads == 2
    cfg.save_pretrained(tmp_path)
    with open(tmp_path / "config.json") as f:
        assert json.load(f)["num_key_value_heads"] == 2
    assert load_model_config(str(tmp_path)).num_key_value_heads == 2
    assert LlamaConfig.from_pretrained(tmp_path).num_key_value_heads == 2
    with pytest.raises(ValueError, match="must divide"):
        LlamaConfig(num_attention_heads=4, num_key_value_heads=3)


def _llama_config_files():
    files = sorted(glob.glob(os.path.join(REPO, "configs", "*.json")))
    files += [os.path.join(GOLDEN, d, "config.json")
              for d in ("ckpt_read_by_reference", "ckpt_written_by_reference")]
    out = []
    for f in files:
        with open(f) as fh:
            if json.load(fh).get("model_type", "llama") == "llama":
                out.append(f)
    return out


def test_existing_configs_keep_square_kv():
    files = _llama_config_files()
    assert len(files) >= 17
    for f in files:
        cfg = load_model_config(f)
        with open(f) as fh:
            explicit = json.load(fh).get("num_key_value_heads")
        hd = cfg.hidden_size // cfg.num_attention_heads
        want_nkv = explicit or cfg.num_attention_heads
        assert cfg.num_key_value_heads == want_nkv, f
        cfg.num_hidden_layers = 1      # shapes only, on the meta device
        cfg.vocab_size = 16
        with torch.device("meta"):
            attn = LlamaForCausalLM(cfg).model.layers[0].self_attn
        assert attn.q_proj.weight.shape == (cfg.hidden_size, cfg.hidden_size), f
        assert attn.k_proj.weight.shape == (want_nkv * hd, cfg.hidden_size), f
        assert attn.v_proj.weight.shape == (want_nkv * hd, cfg.hidden_size), f
        if explicit is None:
            assert attn.k_proj.weight.shape[0] == attn.k_proj.weight.shape[1], f
    gqa = load_model_config(os.path.join(REPO, "configs", "llama_1b_gqa.json"))
    assert (gqa.num_attention_heads, gqa.num_key_value_heads) == (32, 8)


# -- op -----------------------------------------------------------------------

@pytest.mark.parametrize("causal", [True, False])
def test_flash_attention_cpu_equals_repeat_then_sdpa(causal):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, 4, 24, 16, generator=g, requires_grad=True)
    k = torch.randn(2, 2, 24, 16, generator=g, requires_grad=True)
    v = torch.randn(2, 2, 24, 16, generator=g, requires_grad=True)
    dout = torch.randn(2, 4, 24, 16, generator=g)
    out = ops.flash_attention(q, k, v, causal=causal)
    out.backward(dout)
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(
        q2, k2.repeat_interleave(2, dim=1), v2.repeat_interleave(2, dim=1),
        is_causal=causal)
    ref.backward(dout)
    assert k.grad.shape == k.shape and v.grad.shape == v.shape
    for a, b in ((out, ref), (q.grad, q2.grad), (k.grad, k2.grad), (v.grad, v2.grad)):
        assert (a - b).abs().max() <= 1e-6
    # head h reads kv head h // n_rep, not h % nkv: heads 0 and 1 share kv 0
    alt = F.scaled_dot_product_attention(q2, k2.repeat(1, 2, 1, 1), v2.repeat(1, 2, 1, 1),
                                         is_causal=causal)
    assert (out - alt).abs().max() > 1e-3
    with pytest.raises(ValueError, match="must divide"):
        ops.flash_attention(q, torch.randn(2, 3, 24, 16), torch.randn(2, 3, 24, 16))


def test_rope_torch_fewer_kv_heads():
    g = torch.Generator().manual_seed(4)
    q = torch.randn(1, 4, 10, 16, generator=g)
    k = torch.randn(1, 2, 10, 16, generator=g)
    cos, sin = ops.build_rope_cache(8, 10)      # partial rotary: tail passes
    qo, ko = ops.rope(q, k, cos, sin)
    assert qo.shape == q.shape and ko.shape == k.shape
    _, ko_full = ops.rope(k.repeat_interleave(2, 1), k.repeat_interleave(2, 1), cos, sin)
    assert torch.equal(ko_full[:, ::2], ko)
    assert torch.equal(ko[..., 8:], k[..., 8:])


# -- HF parity ----------------------------------------------------------------

def _hf_tiny():
    import transformers

    hf_cfg = transformers.LlamaConfig(
        vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64,
        rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False,
        attention_bias=False, bos_token_id=0, eos_token_id=1, pad_token_id=None)
    # HF's default attention (repeat_kv + SDPA) is the same arithmetic as this
    # project's CPU path, so logits can be compared with torch.equal; its
    # "eager" matmul+softmax differs in the last ulp, for multi-head too
    hf_cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    return transformers.LlamaForCausalLM(hf_cfg).float().eval()


def _same_logits_and_loss(m1, m2, x, what):
    """the criterion of test_hf_from_pretrained_classmethod_exact: torch.equal
    on the logits; the loss is the shifted cross-entropy of those logits
    (this project's forward returns no logits when given labels)"""
    with torch.no_grad():
        a, b = m1(input_ids=x).logits, m2(input_ids=x).logits
        la, lb = m1(input_ids=x, labels=x).loss, m2(input_ids=x, labels=x).loss
    print(what, "max |dlogits|", (a - b).abs().max().item(), "loss", la.item(), lb.item())
    assert torch.equal(a, b), (what, (a - b).abs().max())
    want = F.cross_entropy(a[:, :-1].reshape(-1, a.shape[-1]), x[:, 1:].reshape(-1))
    assert abs(la.item() - want.item()) <= 1e-5 and abs(lb.item() - want.item()) <= 1e-5, (
        what, la, lb, want)


def test_hf_checkpoint_interchange_exact(tmp_path):
    """HF-written GQA checkpoint -> this project's from_pretrained, and a
    checkpoint written here -> HF's from_pretrained: identical logits, loss."""
    import transformers

    hf = _hf_tiny()
    x = torch.randint(0, 128, (2, 12), generator=torch.Generator().manual_seed(1))
    hf.save_pretrained(tmp_path / "hf")
    ours = LlamaForCausalLM.from_pretrained(tmp_path / "hf").eval()
    assert ours.config.num_key_value_heads == 2
    assert ours.model.layers[0].self_attn.k_proj.weight.shape == (32, 64)
    _same_logits_and_loss(hf, ours, x, "hf->ours")

    torch.manual_seed(5)
    mine = LlamaForCausalLM(tiny_gqa_config()).eval()
    save_pretrained_compat(mine, str(tmp_path / "ours"))
    hf2 = transformers.LlamaForCausalLM.from_pretrained(
        tmp_path / "ours", attn_implementation="sdpa").eval()
    assert hf2.config.num_key_value_heads == 2
    _same_logits_and_loss(mine, hf2, x, "ours->hf")


# -- generate -------------------------------------------------------------------

def test_generate_matches_manual_greedy_gqa():
    torch.manual_seed(0)
    x = torch.randint(2, 128, (1, 5))
    m = LlamaForCausalLM(tiny_gqa_config()).eval()
    out = m.generate(x, max_new_tokens=6, do_sample=False)
    cur = x.clone()
    for _ in range(6):
        with torch.no_grad():
            cur = torch.cat([cur, m(input_ids=cur).logits[:, -1:].argmax(-1)], dim=1)
    assert torch.equal(out, cur)
    # cached K/V keep nkv heads; cached decode equals the full recompute
    with torch.no_grad():
        full = m(input_ids=cur).logits
        pre = m(input_ids=cur[:, :-1], use_cache=True)
        from relora_amd.models.cache_compat import cache_to_legacy
        past = cache_to_legacy(pre.past_key_values)
        for kk, vv in past:
            assert kk.shape == (1, 2, cur.shape[1] - 1, 16) and vv.shape == kk.shape
        step = m(input_ids=cur[:, -1:], past_key_values=pre.past_key_values,
                 use_cache=True).logits
    assert (step[:, -1] - full[:, -1]).abs().max() <= 1e-5


# -- ReLoRA ---------------------------------------------------------------------

def test_relora_merge_and_roundtrip_gqa(tmp_path):
    from relora_amd.relora import ReLoRaModel

    torch.manual_seed(0)
    model = ReLoRaModel(LlamaForCausalLM(tiny_gqa_config()), r=8, lora_alpha=32,
                        lora_dropout=0.0, target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.normal_(std=0.05)
    k_proj = model.wrapped_model.model.layers[0].self_attn.k_proj
    assert k_proj.weight.shape == (32, 64) and k_proj.lora_B.weight.shape == (32, 8)
    x = torch.randint(0, 128, (2, 10), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        before = model(input_ids=x).logits
        model.merge_and_reinit()
        merged = model(input_ids=x).logits
    assert (before - merged).abs().max() <= 1e-5
    model.save_pretrained(str(tmp_path))
    again = ReLoRaModel.from_pretrained(str(tmp_path)).eval()
    with torch.no_grad():
        loaded = again(input_ids=x).logits
    assert torch.equal(merged, loaded)


# -- memory ---------------------------------------------------------------------

def test_memory_counts_kv_heads():
    from relora_amd.utils import memory

    mha = load_model_config(os.path.join(REPO, "configs", "llama_1b.json"))
    gqa = load_model_config(os.path.join(REPO, "configs", "llama_1b_gqa.json"))
    L, H, nh, nkv = 24, 2048, 32, 8
    hd = H // nh
    n_mha, lora_mha = memory.estimate_param_count(mha, lora_r=128)
    n_gqa, lora_gqa = memory.estimate_param_count(gqa, lora_r=128)
    assert n_mha - n_gqa == 2 * L * H * (nh - nkv) * hd
    assert lora_mha - lora_gqa == 2 * L * 128 * (nh - nkv) * hd
    with torch.device("meta"):
        real = sum(p.numel() for p in LlamaForCausalLM(gqa).parameters())
    assert real == n_gqa
    # saved K/V activations shrink too
    assert (memory.estimate_step_bytes(gqa, 8, 2048, lora_r=128)
            < memory.estimate_step_bytes(mha, 8, 2048, lora_r=128))


# -- conditioning of the GPU test's inputs --------------------------------------

@pytest.mark.parametrize("hd", [64, 128, 40])
@pytest.mark.parametrize("nkv", [1, 2])
def test_gpu_inputs_are_well_conditioned(nkv, hd):
    """The bf16-rounded computation itself (no kernel) stays inside the
    project's bounds on the seeds the GPU test uses, so a GPU failure there
    means the kernel, not the inputs."""
    q, k, v, dout = gc.make_inputs(2, 4, nkv, 320, hd)
    r = aw.all_ratios(gc.emulate_gqa(q, k, v, dout), gc.ref_gqa(q, k, v, dout))
    print(f"emulated nkv{nkv} hd{hd} err/bound: {r}")
    assert not gc.failures(r), r
