"""config.qk_norm in the model on the GPU: a 2-layer LLaMA (hidden 256, 4
heads, head_dim 64) wrapped in ReLoRA at r = 32, so the group LoRA op feeds
ops.qk_norm_rope, in bf16 on the HIP path against the same model in fp32 on
the CPU; and with the option off the new extension entries are never
entered."""

import copy

import pytest
import torch

from relora_amd import ops
from relora_amd.models.config import LlamaConfig
from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.ops import hip
from relora_amd.relora import ReLoRaModel

pytestmark = pytest.mark.gpu


def _model(qk_norm, nkv=4):
    cfg = LlamaConfig(vocab_size=128, hidden_size=256, intermediate_size=344,
                      num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=nkv,
                      max_position_embeddings=256, qk_norm=qk_norm)
    torch.manual_seed(0)
    model = ReLoRaModel(LlamaForCausalLM(cfg), r=32, lora_alpha=32, lora_dropout=0.0,
                        target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True).train()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_A" in n or "lora_B" in n:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            if "q_norm" in n or "k_norm" in n:
                p.copy_(1 + 0.25 * torch.randn(p.shape, generator=g))
    return model


@pytest.fixture
def spy(monkeypatch):
    calls = {"fwd": 0, "bwd": 0, "group": 0}
    ext = hip.ext()
    real = {"fwd": ext.qk_norm_rope_fwd, "bwd": ext.qk_norm_rope_bwd,
            "group": ops.lora_linear_group}

    def count(name):
        def wrapped(*a, **kw):
            calls[name] += 1
            return real[name](*a, **kw)
        return wrapped

    monkeypatch.setattr(ext, "qk_norm_rope_fwd", count("fwd"))
    monkeypatch.setattr(ext, "qk_norm_rope_bwd", count("bwd"))
    monkeypatch.setattr(ops, "lora_linear_group", count("group"))
    return calls


@pytest.mark.parametrize("variant", ["mha", "gqa", "checkpointing", "doc_start"])
def test_llama_qk_norm_matches_cpu(variant, spy):
    model = _model(True, nkv=2 if variant == "gqa" else 4)
    model.wrapped_model.model.gradient_checkpointing = variant == "checkpointing"
    x = torch.randint(2, 128, (2, 128), generator=torch.Generator().manual_seed(1))
    kw_cpu, kw_gpu = {}, {}
    if variant == "doc_start":
        x[0, [40, 41, 99]] = 1          # eos = 1: documents end at these tokens
        x[1, [63]] = 1
        ds = ops.doc_starts_from_eos(x, 1)
        kw_cpu, kw_gpu = {"doc_start": ds}, {"doc_start": ds.cuda()}

    cpu = copy.deepcopy(model).float()
    cpu_loss = cpu(input_ids=x, labels=x, **kw_cpu).loss
    cpu_loss.backward()
    assert spy["fwd"] == 0

    gpu = model.to("cuda", torch.bfloat16)
    gpu_loss = gpu(input_ids=x.cuda(), labels=x.cuda(), **kw_gpu).loss
    gpu_loss.backward()
    torch.cuda.synchronize()
    # checkpointing runs every layer's forward a second time
    n_fwd = 4 if variant == "checkpointing" else 2
    assert spy["fwd"] == n_fwd and spy["bwd"] == 2, spy
    assert spy["group"] == 2 * n_fwd, spy      # q/k/v and gate/up per layer

    print(f"qk_norm model {variant} loss cpu {cpu_loss.item():.5f} gpu {gpu_loss.item():.5f}")
    # the bounds of test_gpu_attention_docmask.py::test_llama_doc_start_matches_cpu
    assert abs(cpu_loss.item() - gpu_loss.item()) < 0.1, (cpu_loss, gpu_loss)
    refs = {n: prm.grad for n, prm in cpu.named_parameters() if prm.grad is not None}
    gots = {n: prm.grad for n, prm in gpu.named_parameters() if prm.grad is not None}
    assert refs.keys() == gots.keys() and refs
    assert sum("q_norm" in n or "k_norm" in n for n in refs) == 4
    worst = {}
    for n, ref in refs.items():
        got = gots[n].float().cpu()
        assert torch.isfinite(got).all(), n
        worst[n] = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"qk_norm model {variant} worst grad err / |ref|max: {top}")
    for n, ref in refs.items():
        err = worst[n] * ref.abs().max().item()
        assert err <= 0.03 * ref.abs().max().item() + 0.05, (n, err)
        assert worst[n] <= 0.05, (n, worst[n])


def test_option_off_never_enters_the_new_kernels(spy):
    model = _model(False)
    assert not any("q_norm" in n or "k_norm" in n for n, _ in model.named_parameters())
    x = torch.randint(2, 128, (2, 128), generator=torch.Generator().manual_seed(1)).cuda()
    gpu = model.to("cuda", torch.bfloat16)
    loss = gpu(input_ids=x, labels=x).loss
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert spy["fwd"] == 0 and spy["bwd"] == 0, spy
    assert spy["group"] == 4
