"""The fp8 backward on the CPU: the column-scaled oracle, the trainer flag, the switch."""

import pytest
import torch

from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.ops.quant import quantize_fp8_ref
from relora_amd.relora import ReLoRaLinear, ReLoRaModel
from relora_amd.trainer import parse_args

E4 = torch.float8_e4m3fn


def test_oracle_col_scale_on_hand_built_rows():
    """col_scale = 448 * 2^e: g = x * 2^e exactly, so the codes are those of x * 2^e."""
    x = torch.tensor([[448.0, -17.0, 19.0, 2.0 ** -10], [1.0, -2.0, 3.0, 0.5],
                      [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 5.0]]).to(torch.bfloat16)
    e = torch.tensor([0.0, 1.0, -2.0, 0.0])
    codes, absmax = quantize_fp8_ref(x, col_scale=448 * torch.exp2(e))
    want_codes, want_absmax = quantize_fp8_ref(x.float() * torch.exp2(e))
    assert torch.equal(codes, want_codes) and torch.equal(absmax, want_absmax)
    assert absmax.tolist() == [448.0, 4.0, 0.0, 5.0] and not codes[2].any()
    # ties to even: 34 -> 32, 4.75 -> 5, 2^-10 -> 0, 84 -> 80; the row maximum lands on 448
    assert codes.view(E4).float()[0].tolist() == [448.0, -32.0, 5.0, 0.0]
    assert codes.view(E4).float()[1].tolist() == [112.0, -448.0, 80.0, 56.0]
    # a zero scale silences its column; None leaves the function as it was
    zc, za = quantize_fp8_ref(x, col_scale=torch.tensor([448.0, 448.0, 448.0, 0.0]))
    assert za.tolist() == [448.0, 3.0, 0.0, 1.0] and not zc[:, 3].any()
    assert all(torch.equal(a, b) for a, b in zip(quantize_fp8_ref(x), quantize_fp8_ref(x, None)))
    with pytest.raises(ValueError, match="col_scale must have shape"):
        quantize_fp8_ref(x, col_scale=torch.ones(3))


def test_trainer_flag_needs_quantize_fp8():
    base = ["--synthetic_data", "true", "--batch_size", "4", "--gradient_accumulation", "1"]
    assert parse_args(base + ["--quantize", "fp8"]).fp8_backward is False
    assert parse_args(base + ["--quantize", "fp8", "--fp8_backward", "true"]).fp8_backward is True
    for other in ([], ["--quantize", "mxfp4"]):
        with pytest.raises(ValueError, match="needs --quantize fp8"):
            parse_args(base + other + ["--fp8_backward", "true"])


def test_switch_is_ignored_on_cpu(tiny_llama_config, tmp_path):
    torch.manual_seed(3)
    model = ReLoRaModel(LlamaForCausalLM(tiny_llama_config), r=8, lora_alpha=16, lora_dropout=0.0,
                        target_modules=["attn", "mlp"], keep_original_weights=True, quantize="fp8")
    linears = [m for m in model.modules() if isinstance(m, ReLoRaLinear)]
    with torch.no_grad():
        for m in linears:
            m.lora_B.weight.normal_(std=0.02)
    x = torch.randint(0, tiny_llama_config.vocab_size, (2, 16))
    grads = {}
    for on in (False, True):
        assert model.set_fp8_backward(on) is model and all(m.fp8_backward is on for m in linears)
        model.zero_grad(set_to_none=True)
        model(input_ids=x, labels=x).loss.backward()
        grads[on] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    assert grads[True] and all(torch.equal(a, b) for a, b in zip(grads[True], grads[False]))
    model.save_pretrained(tmp_path / "ckpt")     # the switch is no checkpoint key
    assert "fp8_backward" not in (tmp_path / "ckpt" / "relora_config.json").read_text()
