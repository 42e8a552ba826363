"""The fp8 backward (`quantize_rows_fp8_scaled`, `fused_fp8_gemm_dx`, the module
switch) against the CPU oracle of ops/quant.py and float64.  Helpers and bounds
as test_gpu_fp8_gemm.py: 2^-8 per bf16 rounding, n * 2^-23 * sum|a_i b_i| per
fp32 dot product of length n."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd.ops.quant import quantize_fp8_ref
from test_gpu_fp8_gemm import (BF, E4, F32, U, as_codes, assert_within, d, ext, gen, poison,
                               strided, ternary)


@pytest.mark.parametrize("N", [16, 128, 528, 2000, 4096, 8176,  # lane group; wave, 1/2/4/8 units
                               8208])                           # looping form
@pytest.mark.parametrize("R", [1, 5, 64])
def test_quantize_rows_scaled(R, N):
    """Codes and absmax bit-equal to the oracle: random scales over 2^-12..2^12 with a zero
    entry, a row of zeros wherever there is a row 3, then plain random data."""
    g = gen("qs", R, N)
    ws = (torch.rand(N, generator=g) + 0.5) * torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())
    ws[N // 3] = 0
    x = (torch.randn(R, N, generator=g) * torch.exp2((torch.arange(R) % 9 - 4).float())[:, None]).to(BF)
    x[3:4] = 0
    for dy, s in ((x, ws), (torch.randn(R, N, generator=g).to(BF), torch.rand(N, generator=g) + 0.01)):
        codes_ref, amax_ref = quantize_fp8_ref(dy, col_scale=s)
        codes, amax = ext().quantize_rows_fp8_scaled(dy.cuda(), s.cuda())
        assert torch.equal(amax.cpu().view(torch.int32), amax_ref.view(torch.int32))
        bad = codes.cpu() != codes_ref
        assert not bad.any(), (f"{int(bad.sum())} codes differ, of them "
                               f"{int((codes.cpu().view(E4).float() != codes_ref.view(E4).float()).sum())} in value")
    assert codes_ref.view(E4).float().abs().max() == 448


@pytest.mark.parametrize("change,msg", [
    (lambda x, s: (x[:, :24].contiguous(), s[:24]), "multiple of 16"),
    (lambda x, s: (x, s[:16]), "ws must hold one value"),
    (lambda x, s: (x, s.cpu()), "ws must be on dy's device"),
    (lambda x, s: (x.float(), s), "dy must be bf16")])
def test_quantize_rows_scaled_rejects(change, msg):
    x, s = torch.zeros(4, 32, dtype=BF, device="cuda"), torch.ones(32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        ext().quantize_rows_fp8_scaled(*change(x, s))


@pytest.mark.parametrize("M,K", [(256, 256), (512, 256)])
def test_dx_reads_back_w(M, K):
    """gq = codes of the identity, gs = 448: dx is W's codes, byte by byte (every e4m3 value
    is a bf16 value).  N = 512 runs both buffer parities."""
    wq = torch.randint(0, 256, (M, K), generator=gen("rb", M, K), dtype=torch.uint8)
    wq[(wq & 0x7f) == 0x7f] = 0x38   # no NaN codes
    poison(M, K)
    dx = ext().fused_fp8_gemm_dx(as_codes(torch.eye(M)), torch.full((M,), 448.0, device="cuda"),
                                 wq.cuda(), K)
    bad = ~(d(dx) == wq.view(E4).double())
    assert not bad.any(), f"wrong per tile: {bad.view(M // 256, 256, K // 256, 256).sum(dim=(1, 3)).tolist()}"


@pytest.mark.parametrize("N", [128, 256, 384, 640])
@pytest.mark.parametrize("M,K", [(256, 256), (512, 256), (256, 768), (768, 768)])
def test_dx_exact(M, N, K):
    """Ternary codes, power-of-two scales: all sums exact."""
    g = gen("dx-exact", M, N, K)
    gv, wv = ternary((M, N), g), ternary((N, K), g)
    sg = torch.exp2(torch.randint(0, 2, (M,), generator=g).double())
    ref = (gv @ wv) * sg[:, None]
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    poison(M, K)
    dx = ext().fused_fp8_gemm_dx(as_codes(gv), (448 * sg).float().cuda(), as_codes(wv), K)
    bad = ~(d(dx) == ref)
    assert not bad.any(), f"wrong per tile: {bad.view(M // 256, 256, K // 256, 256).sum(dim=(1, 3)).tolist()}"


def dx_ref(dy, wq, ws):
    """float64 dx of the fused arm and its |.| sum: the fake-quantised g times W's raw codes."""
    gq, gs = quantize_fp8_ref(dy, col_scale=ws)
    gd = gq.view(E4).double() * (gs / torch.full_like(gs, 448.0)).double()[:, None]
    wd = wq.view(E4).double()
    return gq, gs, gd @ wd, gd.abs() @ wd.abs()


@pytest.mark.parametrize("M,N,K", [(768, 384, 768), (512, 640, 1024)])
def test_dx_random(M, N, K):
    g = gen("dx-random", M, N, K)
    wq, ws = quantize_fp8_ref(torch.randn(N, K, generator=g).to(BF))
    gq, gs, ref, S = dx_ref(torch.randn(M, N, generator=g).to(BF), wq, ws)
    args = (gq.cuda(), gs.cuda(), wq.cuda(), K)
    dx = ext().fused_fp8_gemm_dx(*args)
    assert_within(dx, ref, U * ref.abs() + N * F32 * S, "dx")
    assert torch.equal(dx, ext().fused_fp8_gemm_dx(*args))


@pytest.mark.parametrize("M", [256, 200], ids=["fused", "materialize"])
def test_fp8_backward_switch(M):
    """Switch off: the bf16 backward within its bound.  Switch on: M = 256 takes the fp8 dx
    arm (bound with the main term on the fake-quantised g), M = 200 gives the same bits."""
    from relora_amd.relora import ReLoRaLinear
    K, N, r, s = 256, 256, 64, 0.25
    g = gen("bwd-module", M)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="fp8",
                       bias=True, weight_data=torch.randn(N, K, generator=g) * 0.05)
    with torch.no_grad():
        lin.lora_A.weight.copy_(torch.randn(r, K, generator=g) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(N, r, generator=g) * 0.1)
    lin = lin.to(device="cuda", dtype=BF)
    x = torch.randn(M, K, generator=g).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(M, N, generator=g).to(BF).cuda()
    A, B, qw = lin.lora_A.weight, lin.lora_B.weight, lin.weight
    grads = {}
    for on in (False, True):
        lin.fp8_backward = on
        x.grad = A.grad = B.grad = None
        lin(x).backward(dy)
        grads[on] = (x.grad.clone(), A.grad.clone(), B.grad.clone())
    x64, A64, sB64, W64, dy64 = d(x), d(A), s * d(B), d(qw.materialize(BF)), d(dy)
    xa, Aa, sBa, dya = x64.abs(), A64.abs(), sB64.abs(), dy64.abs()
    t, us, xA, dysB = x64 @ A64.t(), dy64 @ sB64, xa @ Aa.t(), dya @ sBa
    lora = us @ A64
    _, _, main8, S8 = dx_ref(dy.cpu(), qw.qdata.cpu().view(N, K), qw.absmax.cpu())
    for on, main, S in ((False, dy64 @ W64, dya @ W64.abs()), (True, main8, S8)):
        if on and M % 256:
            assert all(torch.equal(a, b) for a, b in zip(grads[True], grads[False]))
            continue
        dx, dA, dB = grads[on]
        assert_within(dx, main + lora, U * (main + lora).abs() + U * main.abs() + U * lora.abs()
                      + U * (us.abs() @ Aa) + (N + r) * F32 * (S + dysB @ Aa), f"dx on={on}")
        assert_within(dA, us.t() @ x64, U * (us.t() @ x64).abs() + U * (us.abs().t() @ xa)
                      + (M + N) * F32 * (dysB.t() @ xa), f"dA on={on}")
        assert_within(dB, s * (dy64.t() @ t), U * s * (dy64.t() @ t).abs() + U * s * (dya.t() @ t.abs())
                      + (M + K) * F32 * s * (dya.t() @ xA), f"dB on={on}")
    if M % 256 == 0:   # the arm was taken: e4m3 rounding of g moves dx
        assert not torch.equal(grads[True][0], grads[False][0])


def dx_args():
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return dict(gq=z(256, 128, dt=torch.uint8), gs=z(256, dt=torch.float32),
                wq=z(128, 256, dt=torch.uint8), K=256)


def misaligned(t):
    return torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)[1:1 + t.numel()].view(t.shape)


BAD = {"gq-cpu": ("gq", lambda v: v.cpu(), "gq must be a GPU tensor"),
       "gq-1d": ("gq", lambda v: v.view(-1), "gq must be 2-D"),
       "M-128": ("gq", lambda v: v[:128].contiguous(), "requires M%256==0"),
       "N-64": ("gq", lambda v: v[:, :64].contiguous(), "requires M%256==0"),
       "K-128": ("K", lambda v: 128, "requires M%256==0"),
       "K-0": ("K", lambda v: 0, "must be > 0"),
       "gq-strided": ("gq", strided, "g codes must be contiguous"),
       "gq-dtype": ("gq", lambda v: v.to(torch.int8), "g codes must be uint8"),
       "gq-misaligned": ("gq", misaligned, "16-byte aligned"),
       "gs-cpu": ("gs", lambda v: v.cpu(), "g absmax must be on xq's"),
       "gs-strided": ("gs", strided, "g absmax must be contiguous"),
       "gs-dtype": ("gs", lambda v: v.double(), "g absmax must be fp32"),
       "gs-short": ("gs", lambda v: v[:128].contiguous(), "g absmax must hold one value"),
       "wq-cpu": ("wq", lambda v: v.cpu(), "w codes must be on gq's"),
       "wq-strided": ("wq", strided, "w codes must be contiguous"),
       "wq-dtype": ("wq", lambda v: v.to(torch.int8), "w codes must be uint8"),
       "wq-short": ("wq", lambda v: v[:64].contiguous(), "w codes must hold"),
       "wq-misaligned": ("wq", misaligned, "16-byte aligned")}


@pytest.mark.parametrize("case", sorted(BAD))
def test_fused_fp8_gemm_dx_rejects(case):
    key, change, msg = BAD[case]
    a = dx_args()
    a[key] = change(a[key])
    with pytest.raises(RuntimeError, match=msg):
        ext().fused_fp8_gemm_dx(*a.values())
