"""No GPU: what tests/test_gpu_norms.py and tests/test_gpu_activations.py rest
on.  The float64 references of tests/norm_common.py agree with
F.layer_norm / rmsnorm_torch and with float64 autograd; the offset and
constant rows tell the one-pass variance from the two-pass one at the stated
bound; the integer row-coverage data moves dw by at least 1 for any dropped
row; and the CPU-measured constants behind the intrinsic allowances (rsqrtf,
__expf, erff) are what norm_common.py records."""

import pytest
import torch
import torch.nn.functional as F

import norm_common as nc
from relora_amd.ops import rmsnorm_torch

BF16, FP32 = torch.bfloat16, torch.float32
H_GRID = [1, 7, 8, 9, 12, 100, 504, 512, 513, 520, 2048, 2049, 2056, 4096, 4104, 5461]


def _close(a, b, rtol=1e-11):
    return (a - b).abs().max() <= rtol * b.abs().max().clamp_min(1e-300)


# -- references ---------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 7, 100, 513])
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_rms_reference_matches_autograd(H, dtype):
    eps = 1e-6
    x, w, _, dy = nc.make_rows(5, H, dtype, seed=H)
    _, _, _, dsum = nc.make_rows(5, H, dtype, seed=H + 1)
    ref = nc.rms_reference(x, w, dy, eps, dsum=dsum)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    ir = (xd.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = wd * xd * ir
    gx, gw = torch.autograd.grad(y, (xd, wd), dy.double())
    assert _close(ref["y"], y.detach()) and _close(ref["invrms"], ir.detach().squeeze(-1))
    assert _close(ref["dx"], gx + dsum.double()) and _close(ref["dw"], gw)
    # the project's torch implementation, in float64 (its mean square is fp32)
    assert _close(ref["y"], rmsnorm_torch(x.double(), w.double(), eps), rtol=1e-5)
    for k in ("y", "invrms", "dx", "dw"):
        assert (ref[k + "_bound"] >= 0).all() and ref[k + "_bound"].shape == ref[k].shape


@pytest.mark.parametrize("H", [1, 7, 100, 513])
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_ln_reference_matches_autograd(H, dtype):
    eps = 1e-5
    x, w, b, dy = nc.make_rows(5, H, dtype, seed=H)
    ref = nc.ln_reference(x, w, b, dy, eps)
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    y = F.layer_norm(xd, (H,), wd, bd, eps)
    gx, gw, gb = torch.autograd.grad(y, (xd, wd, bd), dy.double())
    assert _close(ref["y"], y.detach())
    assert _close(ref["mean"], x.double().mean(-1))
    assert _close(ref["invstd"], (x.double().var(-1, unbiased=False) + eps).rsqrt())
    if H > 1:
        assert _close(ref["dx"], gx, rtol=1e-9) and _close(ref["dw"], gw, rtol=1e-9)
    else:           # xhat = 0: dx and dw are 0, up to float64 rounding in autograd
        assert ref["dx"].abs().max() == 0 and gx.abs().max() < 1e-9
        assert ref["dw"].abs().max() == 0 and gw.abs().max() < 1e-9
    assert _close(ref["db"], gb)
    for k in ("y", "mean", "invstd", "dx", "dw", "db"):
        assert (ref[k + "_bound"] >= 0).all() and ref[k + "_bound"].shape == ref[k].shape


# -- the cancellation rows -----------------------------------------------------------

@pytest.mark.parametrize("H", [100, 768])
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_offset_rows_tell_one_pass_from_two_pass(H, dtype):
    """fp32 emulations with torch's sums.  On every offset row the one-pass
    invstd is outside the bound test_gpu_norms.py applies, the two-pass one
    (what layernorm_fwd_kernel computes) inside on every row; on the zero row
    both are exact."""
    eps = 1e-5
    x = nc.special_rows(H, dtype, seed=H)
    w = torch.ones(H, dtype=dtype)
    ref = nc.ln_reference(x, w, torch.zeros_like(w), torch.zeros_like(x), eps)
    one = nc.one_pass_invstd_fp32(x, eps).double()
    mean2, two = nc.two_pass_stats_fp32(x, eps)
    f_one = (one - ref["invstd"]).abs() / ref["invstd_bound"]
    f_two = (two.double() - ref["invstd"]).abs() / ref["invstd_bound"]
    f_mean = (mean2.double() - ref["mean"]).abs() / ref["mean_bound"].clamp_min(1e-300)
    names = nc.SPECIAL_ROWS[dtype]
    for i, name in enumerate(names):
        print(f"H{H} {dtype} {name}: one-pass {f_one[i]:.3g} two-pass {f_two[i]:.3g} of the "
              f"bound; invstd rel err one-pass {(one[i] / ref['invstd'][i] - 1).abs():.3g}")
    assert names[3] == "zeros" and f_one[3] <= 1 and f_two[3] <= 1
    # Which rows separate the formulas.  The one-pass sums are exact, and so
    # is its variance, where every partial sum fits 24 bits: 256 + {0, 2} at
    # H = 100 (integers, sum x^2 < 2^24; at 768 it is not).  Sums of one
    # repeated value are exact wherever the summation doubles, and bf16
    # squares have 16 bits to spare, so a constant row separates them only for
    # some summation orders: with torch's it does for fp32 at H = 768.
    separates = {(BF16, 100): [1], (BF16, 768): [0, 1],
                 (FP32, 100): [0, 1], (FP32, 768): [0, 1, 2]}[(dtype, H)]
    assert (f_one[separates] > 1).all(), f_one
    assert (f_two <= 1).all() and (f_mean <= 1).all(), (f_two, f_mean)


# -- row coverage data -----------------------------------------------------------------

@pytest.mark.parametrize("layernorm", [False, True])
@pytest.mark.parametrize("M,H", [(1, 24), (65, 24), (130, 256), (16385, 8)])
def test_coverage_data_sees_a_dropped_row(M, H, layernorm):
    x, dy = nc.coverage_case(M, H, BF16, layernorm)
    xd = x.double()
    assert (xd.abs() == 1).all()                   # mean(x^2) = 1, exactly in bf16
    if layernorm:
        assert not xd.sum(-1).any()                # mean 0, so variance 1
    assert torch.equal(dy.double(), dy.double().round()) and dy.double().abs().max() <= 3
    dw, db = nc.coverage_reference(x, dy)
    term = dy.double() * xd                        # row r's share of dw
    # dropping row r moves dw[c] by term[r, c], doubling it by as much the other way
    assert (term.abs() >= 1).all()
    assert (term.sign() == term[0].sign()).all()   # all one way per column: no cancelling
    assert (dw.abs() >= M).all() and term.abs().sum(0).max() < 2 ** 24
    assert torch.equal(dw, term.sum(0))


# -- measured constants ------------------------------------------------------------------

def test_rsqrt_allowance_is_four_times_the_cpu_error():
    """the arguments of rsqrtf in the GPU tests: mean square + eps and
    variance + eps of every case builder, and a sweep over 24 decades"""
    args = [torch.logspace(-12, 12, 200001, dtype=torch.float64)]
    for dtype in (BF16, FP32):
        for H in H_GRID:
            x = nc.make_rows(5, H, dtype, seed=H)[0].double()
            for eps in (0.0, 1e-6, 1e-5, 1e-2):
                args += [x.pow(2).mean(-1) + eps, x.var(-1, unbiased=False) + eps]
        sp = nc.special_rows(768, dtype).double()
        args += [sp.pow(2).mean(-1) + 1e-5, sp.var(-1, unbiased=False) + 1e-5]
    measured = nc.measure_rsqrt(torch.cat(args))
    print(f"rsqrt fp32 on the CPU: {measured:.3f} * 2^-24")
    assert 0.8 * nc.RSQRT_MEASURED <= measured <= nc.RSQRT_MEASURED
    assert nc.RSQRT_REL == 4 * nc.RSQRT_MEASURED * 2.0 ** -24


def test_activation_allowances_are_four_times_the_cpu_error():
    """the fp32 formulas of swiglu.hip by torch on the CPU against float64,
    over the bf16 sweep and the fp32 grid with every (u, dy) pair"""
    worst = dict.fromkeys(nc.ACT_MEASURED, 0.0)
    for g in (nc.bf16_sweep(), nc.fp32_grid()):
        for u in nc.SWEEP_U:
            for dy in nc.SWEEP_DY:
                m = nc.measure_activation_units(g, torch.full_like(g, u), torch.full_like(g, dy))
                worst = {k: max(worst[k], m[k]) for k in worst}
    print("fp32 formulas on the CPU, in unit * 2^-24:", worst)
    for k, v in worst.items():
        assert 0.8 * nc.ACT_MEASURED[k] <= v <= nc.ACT_MEASURED[k], (k, v)
        assert nc.ACT_UNITS[k] == 4 * nc.ACT_MEASURED[k]


def test_bf16_sweep_is_every_zero_or_normal_pattern():
    v = nc.bf16_sweep()
    assert v.numel() == 65536 - 256 - 254
    f = v.float()
    assert torch.isfinite(f).all()
    assert ((f == 0) | (f.abs() >= 2.0 ** -126)).all()
    assert v.view(torch.int16).unique().numel() == v.numel()
    # the float64 references are finite on all of it
    for u in nc.SWEEP_U:
        ref, _ = nc.act_reference(v, torch.full_like(v, u), torch.full_like(v, -0.5))
        assert all(torch.isfinite(r).all() for r in ref.values())
