"""`--quantize fp8` on the CPU: oracle, QuantizedWeight, model wrap, checkpoints, parser."""

import copy

import pytest
import torch

from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.ops.quant import QuantizedWeight, dequantize_fp8_ref, quantize_fp8_ref
from relora_amd.relora import ReLoRaLinear, ReLoRaModel
from relora_amd.trainer import parse_args


def exact_rows(R, K, seed=0):
    """Rows on the e4m3 grid times 2^e, e per row and of either sign, 448*2^e once
    a row: inv is a power of two and v*inv exact, so quantising is lossless."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[grid.isfinite() & (grid.abs() < 448)]   # subnormals and -0 included
    v = grid[torch.randint(0, grid.numel(), (R, K), generator=g)]
    v[torch.arange(R), torch.arange(R) % K] = 448.0 * (1 - 2 * (torch.arange(R) % 2))
    e = (torch.arange(R) % 9 - 4).float()               # 2^-4 .. 2^4, bf16-exact values
    return v * torch.exp2(e).unsqueeze(1)


@pytest.mark.parametrize("R,K", [(1, 16), (5, 208), (64, 128)])
def test_oracle_round_trip_is_identity_on_exact_rows(R, K):
    x = exact_rows(R, K)
    x[R // 2] = 0 if R > 1 else x[0]          # a row of zeros encodes to zeros
    codes, absmax = quantize_fp8_ref(x)
    assert torch.equal(absmax, x.abs().amax(dim=1))
    assert codes.view(torch.float8_e4m3fn).float().abs().max() == 448
    assert torch.equal(dequantize_fp8_ref(codes, absmax), x)


def test_quantized_weight_fp8_cpu_and_model_cast():
    w = torch.randn(48, 40, generator=torch.Generator().manual_seed(1))
    qw = QuantizedWeight(w, "fp8")
    assert (qw.qdata.dtype, qw.qdata.shape, qw.absmax.shape) == (torch.uint8, (48 * 40,), (48,))
    want = dequantize_fp8_ref(*quantize_fp8_ref(w))
    assert torch.equal(qw.materialize(), want)
    qw = qw.to(torch.bfloat16)            # a model-wide cast keeps the fp32 scales
    assert qw.absmax.dtype == torch.float32 and qw.qdata.dtype == torch.uint8
    assert torch.equal(qw.materialize(torch.float32), want)
    qw.requantize_(want * 2)
    assert torch.equal(qw.materialize(torch.float32), want * 2)


WRAP = dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["attn", "mlp"],
            keep_original_weights=True)


def test_fp8_model_equals_dense_model_on_dequantised_weights(tiny_llama_config, tmp_path):
    torch.manual_seed(2)
    base = LlamaForCausalLM(tiny_llama_config)
    dense, fp8 = ReLoRaModel(copy.deepcopy(base), **WRAP), ReLoRaModel(base, quantize="fp8", **WRAP)
    with torch.no_grad():
        dense_params = dict(dense.named_parameters())
        for n, pq in fp8.named_parameters():
            if "lora_" in n:
                pq.add_(torch.randn_like(pq) * 0.02)
                dense_params[n].copy_(pq)
        fp8_modules = dict(fp8.named_modules())
        for name, md in dense.named_modules():
            if isinstance(md, ReLoRaLinear):
                assert fp8_modules[name].weight.mode == "fp8"
                md.weight.copy_(dequantize_fp8_ref(*quantize_fp8_ref(md.weight)))
    x = torch.randint(0, tiny_llama_config.vocab_size, (2, 16))
    dense.eval(), fp8.eval()
    with torch.no_grad():
        assert torch.equal(dense(input_ids=x, labels=x).loss, fp8(input_ids=x, labels=x).loss)

    fp8.save_pretrained(tmp_path / "ckpt")
    back = ReLoRaModel.from_pretrained(str(tmp_path / "ckpt")).eval()
    assert all(m.quantize == "fp8" for m in back.modules() if isinstance(m, ReLoRaLinear))
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in fp8.state_dict().items())
    with torch.no_grad():
        assert torch.equal(fp8(input_ids=x, labels=x).loss, back(input_ids=x, labels=x).loss)


def test_parser_and_mode_validation():
    base = ["--synthetic_data", "true", "--batch_size", "4", "--gradient_accumulation", "1"]
    assert parse_args(base + ["--quantize", "fp8"]).quantize == "fp8"
    with pytest.raises(SystemExit):
        parse_args(base + ["--quantize", "fp4"])
    with pytest.raises(ValueError):
        ReLoRaLinear(16, 16, r=4, quantize="fp4")
    with pytest.raises(ValueError):
        QuantizedWeight(torch.zeros(4, 16), "fp4")
