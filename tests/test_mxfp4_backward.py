"""The MXFP4 backward on the CPU: the e4m3 transcode oracle, the trainer flag, the switch."""

import pytest
import torch

from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.ops.quant import (QuantizedWeight, dequantize_mxfp4_ref, quantize_mxfp4_ref,
                                  transcode_mxfp4_e4m3_ref)
from relora_amd.relora import ReLoRaLinear, ReLoRaModel
from relora_amd.trainer import parse_args

E4 = torch.float8_e4m3fn
BASE = [0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C]   # e4m3 bytes of 0 .5 1 1.5 2 3 4 6
# magnitude bytes of the 8 e2m1 magnitudes at a spread E - s: units of 2^-9 once subnormal.
# 15 .. 18 round to nearest, ties to even (1.5 -> 2, 0.5 -> 0, 0.75 -> 1, 0.375 -> 0)
WANT = {0: [0] + [b + 0x30 for b in BASE[1:]], 6: BASE,
        13: [0, 2, 4, 6, 8, 12, 16, 20], 14: [0, 1, 2, 3, 4, 6, 8, 12],
        15: [0, 0, 1, 2, 2, 3, 4, 6], 16: [0, 0, 0, 1, 1, 2, 2, 3],
        17: [0, 0, 0, 0, 0, 1, 1, 2], 18: [0, 0, 0, 0, 0, 0, 0, 1],
        19: [0] * 8, 40: [0] * 8, 200: [0] * 8}
ALL16 = (torch.arange(0, 16, 2) | (torch.arange(1, 16, 2) << 4)).to(torch.uint8).repeat(2)


def test_transcode_on_hand_built_blocks():
    """One row per spread, every code twice a block, stripe 0 at E = 210; stripe 1 all zero.
    The all-zero result starts at a spread of 19: 6 * 2^(6-17) is 1.5 subnormal steps and
    6 * 2^(6-18) is 0.75, both of which round up."""
    E, spreads = 210, sorted(WANT)
    codes = torch.cat([ALL16.repeat(len(spreads), 1), torch.zeros(len(spreads), 16, dtype=torch.uint8)], 1)
    scales = torch.tensor([[E - s, 127] for s in spreads], dtype=torch.uint8)
    B, emax = transcode_mxfp4_e4m3_ref(codes, scales, 64)
    assert B.shape == (len(spreads), 64) and emax.tolist() == [E, 127]
    for row, s in zip(B, spreads):
        want = WANT[s] + [b | 0x80 for b in WANT[s]]     # the sign is kept, -0 stays -0
        assert row[:32].tolist() == want * 2, f"spread {s}"
    assert not B[:, 32:].any()
    assert not ((B & 0x7F) == 0x7F).any()
    w = dequantize_mxfp4_ref(codes, scales, 64)
    back = B.view(E4).float() * torch.exp2(emax.float() - 133).repeat_interleave(32)
    exact = torch.tensor([s <= 14 for s in spreads])
    assert torch.equal(back[exact], w[exact]) and not torch.equal(back[~exact], w[~exact])
    with pytest.raises(ValueError, match="need K % 32 == 0"):
        transcode_mxfp4_e4m3_ref(codes, scales[:, :1], 64)


def test_stripe_exponents_are_cached_outside_the_state_dict():
    w = torch.randn(64, 96, generator=torch.Generator().manual_seed(5))
    qw = QuantizedWeight(w, "mxfp4")
    emax = quantize_mxfp4_ref(w)[1].amax(0)
    assert torch.equal(qw.stripe_emax(), emax) and qw.stripe_emax() is qw.stripe_emax()
    assert sorted(qw.state_dict()) == ["absmax", "qdata"]
    state = {k: v.clone() for k, v in qw.state_dict().items()}
    qw.requantize_(w * 4)
    assert torch.equal(qw.stripe_emax(), emax + 2)
    qw.load_state_dict(state)
    assert torch.equal(qw.stripe_emax(), emax)


def test_trainer_flag_needs_quantize_mxfp4():
    base = ["--synthetic_data", "true", "--batch_size", "4", "--gradient_accumulation", "1"]
    assert parse_args(base + ["--quantize", "mxfp4"]).mxfp4_backward is False
    assert parse_args(base + ["--quantize", "mxfp4", "--mxfp4_backward", "true"]).mxfp4_backward is True
    for other in ([], ["--quantize", "fp8"]):
        with pytest.raises(ValueError, match="needs --quantize mxfp4"):
            parse_args(base + other + ["--mxfp4_backward", "true"])


def test_switch_is_ignored_on_cpu(tiny_llama_config, tmp_path):
    torch.manual_seed(3)
    model = ReLoRaModel(LlamaForCausalLM(tiny_llama_config), r=8, lora_alpha=16, lora_dropout=0.0,
                        target_modules=["attn", "mlp"], keep_original_weights=True, quantize="mxfp4")
    linears = [m for m in model.modules() if isinstance(m, ReLoRaLinear)]
    with torch.no_grad():
        for m in linears:
            m.lora_B.weight.normal_(std=0.02)
    x = torch.randint(0, tiny_llama_config.vocab_size, (2, 16))
    grads = {}
    for on in (False, True):
        model.set_fp8_backward(on)
        model.zero_grad(set_to_none=True)
        model(input_ids=x, labels=x).loss.backward()
        grads[on] = [p.grad.clone() for p in model.parameters() if p.grad is not None]
    assert grads[True] and all(torch.equal(a, b) for a, b in zip(grads[True], grads[False]))
    model.save_pretrained(tmp_path / "ckpt")     # the switch is no checkpoint key
    assert "backward" not in (tmp_path / "ckpt" / "relora_config.json").read_text()
