"""`--quantize mxfp4` on the CPU: the format's reference, QuantizedWeight, model wrap,
checkpoints, parser."""

import copy

import pytest
import torch

from relora_amd.models.llama import LlamaForCausalLM
from relora_amd.ops.quant import QuantizedWeight, dequantize_mxfp4_ref, quantize_mxfp4_ref
from relora_amd.relora import ReLoRaLinear, ReLoRaModel
from relora_amd.trainer import parse_args

GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6])
ALL = torch.cat([GRID, -GRID])               # element i has code i (-0 is code 8)
TIES = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5])
TIES_TO = torch.tensor([0, 1, 1, 2, 2, 4, 4.])  # the even code of the two neighbours
SAT = torch.tensor([7.5, 7, 6.5, -7, 6.25, -7.75])


def hand_rows():
    """-> (w [6, 64], want [6, 64], scale bytes [6, 2]).  Blocks of 32 at unit scale,
    amax in front so that w[:, :53] (a short last block of 21) keeps it:
    every code twice; 6 then the ties of either sign; the same under amax 4, a power
    of two; values in (6, 8) saturating.  A row is two blocks at different scales."""
    pad = lambda v: torch.cat([v, torch.zeros(32 - v.numel())])  # noqa: E731
    every = (torch.cat([ALL[1:], ALL[:1], ALL]),) * 2
    ties6 = pad(torch.cat([GRID[7:], TIES, -TIES])), pad(torch.cat([GRID[7:], TIES_TO, -TIES_TO]))
    ties4 = (pad(torch.cat([GRID[6:7], TIES[:6], -TIES[:6]])),
             pad(torch.cat([GRID[6:7], TIES_TO[:6], -TIES_TO[:6]])))
    sat = torch.cat([SAT, ALL, ALL[:10]]), torch.cat([6 * SAT.sign(), ALL, ALL[:10]])
    zero = (torch.zeros(32),) * 2
    plan = [(every, 0, ties6, -3), (ties6, 5, every, -7), (ties4, -1, sat, 3),
            (sat, -10, ties4, 4), (zero, 0, every, 1), (every, -2, zero, 0)]
    w, want = (torch.stack([torch.cat([a[i] * 2.0 ** ea, b[i] * 2.0 ** eb])
                            for a, ea, b, eb in plan]) for i in (0, 1))
    return w, want, torch.tensor([[127 + ea, 127 + eb] for _, ea, _, eb in plan], dtype=torch.uint8)


@pytest.mark.parametrize("K", [64, 53])
def test_reference_on_hand_built_rows(K):
    w, want, scales = hand_rows()
    codes, got_scales = quantize_mxfp4_ref(w[:, :K])
    assert codes.shape == (6, 32) and torch.equal(got_scales, scales)
    assert torch.equal(dequantize_mxfp4_ref(codes, scales, K), want[:, :K])
    # low nibble = lower k, the sign bit is kept: codes 1..15, 0 then 0..15 in row 0
    nib = torch.stack((codes[0, :16] & 15, codes[0, :16] >> 4), 1).view(-1)
    assert nib.tolist() == list(range(1, 16)) + [0] + list(range(16))
    if K == 53:  # the padding of the short block encodes as zero codes
        assert int(codes[:, 27:].max()) == 0 and int((codes[:, 26] >> 4).max()) == 0
        assert dequantize_mxfp4_ref(codes, scales, K, torch.bfloat16).shape == (6, 53)


def test_quantized_weight_mxfp4_cpu_and_model_cast():
    w = torch.randn(48, 40, generator=torch.Generator().manual_seed(1))
    qw = QuantizedWeight(w, "mxfp4")
    assert (qw.qdata.dtype, qw.qdata.shape) == (torch.uint8, (48, 32))
    assert (qw.absmax.dtype, qw.absmax.shape) == (torch.uint8, (48, 2))
    want = dequantize_mxfp4_ref(*quantize_mxfp4_ref(w), 40)
    assert torch.equal(qw.materialize(), want) and not torch.equal(want, w)
    qw = qw.to(torch.bfloat16)            # a model-wide cast leaves the scale bytes alone
    assert qw.absmax.dtype == torch.uint8 and qw.qdata.dtype == torch.uint8
    assert torch.equal(qw.materialize(torch.float32), want)
    qw.requantize_(want * 2)
    assert torch.equal(qw.materialize(torch.float32), want * 2)
    assert "mode=mxfp4" in repr(qw)


WRAP = dict(r=8, lora_alpha=16, lora_dropout=0.0, target_modules=["attn", "mlp"],
            keep_original_weights=True)


def test_mxfp4_model_equals_dense_model_on_dequantised_weights(tiny_llama_config, tmp_path):
    torch.manual_seed(2)
    base = LlamaForCausalLM(tiny_llama_config)
    dense, mx = ReLoRaModel(copy.deepcopy(base), **WRAP), ReLoRaModel(base, quantize="mxfp4", **WRAP)
    with torch.no_grad():
        dense_params = dict(dense.named_parameters())
        for n, pq in mx.named_parameters():
            if "lora_" in n:
                pq.add_(torch.randn_like(pq) * 0.02)
                dense_params[n].copy_(pq)
        mx_modules = dict(mx.named_modules())
        for name, md in dense.named_modules():
            if isinstance(md, ReLoRaLinear):
                assert mx_modules[name].weight.mode == "mxfp4"
                md.weight.copy_(dequantize_mxfp4_ref(*quantize_mxfp4_ref(md.weight), md.in_features))
    x = torch.randint(0, tiny_llama_config.vocab_size, (2, 16))
    dense.eval(), mx.eval()
    with torch.no_grad():
        assert torch.equal(dense(input_ids=x, labels=x).loss, mx(input_ids=x, labels=x).loss)

    mx.save_pretrained(tmp_path / "ckpt")
    back = ReLoRaModel.from_pretrained(str(tmp_path / "ckpt")).eval()
    assert all(m.quantize == "mxfp4" for m in back.modules() if isinstance(m, ReLoRaLinear))
    state = back.state_dict()
    assert all(v.dtype == state[k].dtype and torch.equal(v, state[k]) for k, v in mx.state_dict().items())
    with torch.no_grad():
        assert torch.equal(mx(input_ids=x, labels=x).loss, back(input_ids=x, labels=x).loss)


def test_parser_and_constructors_accept_mxfp4():
    base = ["--synthetic_data", "true", "--batch_size", "4", "--gradient_accumulation", "1"]
    assert parse_args(base + ["--quantize", "mxfp4"]).quantize == "mxfp4"
    assert ReLoRaLinear(32, 16, r=4, quantize="mxfp4").weight.mode == "mxfp4"
    assert QuantizedWeight(torch.zeros(4, 16), "mxfp4").absmax.tolist() == [[127]] * 4
