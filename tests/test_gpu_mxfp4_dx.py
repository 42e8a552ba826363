"""The MXFP4 backward (`fused_mxfp4_gemm_dx`, the module switch) against the CPU oracle of
ops/quant.py and float64.  Helpers and bounds as test_gpu_fp8_dx.py: 2^-8 per bf16 rounding,
n * 2^-23 * sum|a_i b_i| per fp32 dot product of length n."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd.ops.quant import quantize_fp8_ref, quantize_mxfp4_ref, transcode_mxfp4_e4m3_ref
from test_gpu_fp8_dx import misaligned
from test_gpu_fp8_gemm import (BF, E4, F32, U, as_codes, assert_within, d, ext, gen, poison,
                               strided, ternary)


def pack(code):
    """e2m1 codes [N,K] -> bytes [N,K/2], the low nibble the lower k."""
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)


def b_ref(codes, scales, K):
    """float64 W as the kernel multiplies it: the reference B times its stripe's power of two."""
    B, emax = transcode_mxfp4_e4m3_ref(codes, scales, K)
    return B.view(E4).double() * torch.exp2(emax.double() - 133).repeat_interleave(32), emax


def run(gq, gs, codes, scales, emax, K):
    return ext().fused_mxfp4_gemm_dx(gq.cuda(), gs.cuda(), codes.cuda(), scales.cuda(), emax.cuda(),
                                     codes.shape[0], K)


def per_tile(bad, M, K):
    return f"wrong per tile: {bad.view(M // 256, 256, K // 256, 256).sum(dim=(1, 3)).tolist()}"


@pytest.mark.parametrize("M,K", [(256, 256), (512, 256)])
def test_dx_reads_back_b(M, K):
    """gq = codes of the identity, gs = 448: dx is the staged image, byte for byte, times
    2^(E-133).  All 16 codes; every stripe has a block at spread 0 and the others at
    0, 3, 8, 14 (exact), 15 (ties) or 19 (flushed).  N = 512 runs both buffer parities."""
    g = gen("mx-rb", M, K)
    codes = pack(torch.randint(0, 16, (M, K), generator=g))
    spread = torch.tensor([0, 3, 8, 14, 15, 19])[torch.randint(0, 6, (M, K // 32), generator=g)]
    spread[torch.randint(0, M, (K // 32,), generator=g), torch.arange(K // 32)] = 0
    scales = (torch.randint(120, 136, (K // 32,), generator=g)[None] - spread).to(torch.uint8)
    ref, emax = b_ref(codes, scales, K)
    poison(M, K)
    dx = run(as_codes(torch.eye(M)), torch.full((M,), 448.0), codes, scales, emax, K)
    bad = ~(d(dx) == ref)
    assert not bad.any(), per_tile(bad, M, K)


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("N", [128, 256, 384, 640])
@pytest.mark.parametrize("M", [256, 512, 768])
def test_dx_exact(M, N, K):
    """Ternary g, W = +-1 * 2^{0,1} or 0, power-of-two row scales: all sums exact.  NT 1..5,
    both buffer parities, grids on both sides of the XCD remap."""
    g = gen("mx-exact", M, N, K)
    gv, wt = ternary((M, N), g), ternary((N, K), g)
    codes = pack(torch.where(wt == 0, 0, torch.where(wt > 0, 2, 10)))
    scales = torch.randint(127, 129, (N, K // 32), generator=g).to(torch.uint8)
    sg = torch.exp2(torch.randint(0, 2, (M,), generator=g).double())
    wv, emax = b_ref(codes, scales, K)
    ref = (gv @ wv) * sg[:, None]
    assert torch.equal(wv, wt * torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1))
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    poison(M, K)
    dx = run(as_codes(gv), (448 * sg).float(), codes, scales, emax, K)
    bad = ~(d(dx) == ref)
    assert not bad.any(), per_tile(bad, M, K)


def dx_ref(dy, codes, scales, K):
    """float64 dx of the fused arm and its |.| sum: the fake-quantised dy times the reference B."""
    gq, gs = quantize_fp8_ref(dy)
    gd = gq.view(E4).double() * (gs / torch.full_like(gs, 448.0)).double()[:, None]
    wd, emax = b_ref(codes, scales, K)
    return gq, gs, emax, gd @ wd, gd.abs() @ wd.abs()


@pytest.mark.parametrize("M,N,K", [(768, 384, 768), (512, 640, 1024)])
def test_dx_random(M, N, K):
    """Normal W against float64.  Then rows 2^20 apart, blocks at every spread up to 21: the
    matrix instruction's sum is no fp32 dot product there (2 of 589824 outputs at 1.2x the
    bound, the same bits in fused_fp8_gemm_dx), so the check is that kernel on the reference B."""
    g = gen("mx-random", M, N, K)
    w, dy = torch.randn(N, K, generator=g), torch.randn(M, N, generator=g).to(BF)
    codes, scales = quantize_mxfp4_ref(w.to(BF))
    gq, gs, emax, ref, S = dx_ref(dy, codes, scales, K)
    dx = run(gq, gs, codes, scales, emax, K)
    assert_within(dx, ref, U * ref.abs() + N * F32 * S, "dx")
    assert torch.equal(dx, run(gq, gs, codes, scales, emax, K))
    wide = w * torch.exp2(torch.randint(-10, 11, (N, 1), generator=g).float())
    codes, scales = quantize_mxfp4_ref(wide.to(BF))
    B, emax = transcode_mxfp4_e4m3_ref(codes, scales, K)
    assert int((emax.int()[None] - scales.int()).max()) >= 19
    dx8 = ext().fused_fp8_gemm_dx(gq.cuda(), gs.cuda(), B.cuda(), K)
    bad = ~(d(run(gq, gs, codes, scales, emax, K)) == d(dx8) * torch.exp2(emax.double() - 133).repeat_interleave(32))
    assert not bad.any(), per_tile(bad, M, K)


@pytest.mark.parametrize("M", [256, 200], ids=["fused", "materialize"])
def test_mxfp4_backward_switch(M):
    """Switch off: dx within the bf16 bound.  Switch on: M = 256 takes the new arm (main term
    on the fake-quantised operands), M = 200 the same bits; dA and dB the same bits always."""
    from relora_amd.relora import ReLoRaLinear
    K, N, r, s = 256, 256, 64, 0.25
    g = gen("mx-bwd-module", M)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="mxfp4",
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
    assert all(torch.equal(a, b) for a, b in zip(grads[True][1:], grads[False][1:]))
    if M % 256:
        assert torch.equal(grads[True][0], grads[False][0])
    else:   # the arm was taken: e4m3 rounding of dy moves dx
        assert not torch.equal(grads[True][0], grads[False][0])
    A64, sB64, W64, dy64 = d(A), s * d(B), d(qw.materialize(BF)), d(dy)
    us, Aa, dysB = dy64 @ sB64, A64.abs(), dy64.abs() @ sB64.abs()
    lora = us @ A64
    _, _, _, main8, S8 = dx_ref(dy.cpu(), qw.qdata.cpu(), qw.absmax.cpu(), K)
    for on, main, S in ((False, dy64 @ W64, dy64.abs() @ W64.abs()), (True, main8, S8)):
        if not on or M % 256 == 0:
            assert_within(grads[on][0], main + lora, U * (main + lora).abs() + U * main.abs()
                          + U * lora.abs() + U * (us.abs() @ Aa) + (N + r) * F32 * (S + dysB @ Aa),
                          f"dx on={on}")


def dx_args():
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return dict(gq=z(256, 128), gs=z(256, dt=torch.float32), wq=z(128, 128), wscales=z(128, 8),
                emax=z(8), N=128, K=256)


BAD = {"gq-cpu": ("gq", lambda v: v.cpu(), "gq must be a GPU tensor"),
       "gq-1d": ("gq", lambda v: v.view(-1), "gq must be 2-D"),
       "M-128": ("gq", lambda v: v[:128].contiguous(), "requires M%256==0"),
       "N-64": ("N", lambda v: 64, "N%128==0"), "K-128": ("K", lambda v: 128, "K%256==0"),
       "gq-strided": ("gq", strided, "g codes must be contiguous"),
       "gq-size": ("gq", lambda v: v[:, :64].contiguous(), "g codes must hold M\\*N"),
       "gq-misaligned": ("gq", misaligned, "g codes must be 16-byte aligned"),
       "gs-dtype": ("gs", lambda v: v.double(), "g absmax must be fp32"),
       "gs-short": ("gs", lambda v: v[:128].contiguous(), "g absmax must hold one value"),
       "wq-cpu": ("wq", lambda v: v.cpu(), "w codes must be on gq's"),
       "wq-short": ("wq", lambda v: v[:64].contiguous(), "w codes must hold N\\*K/2"),
       "wq-misaligned": ("wq", misaligned, "w codes must be 16-byte aligned"),
       "wscales-short": ("wscales", lambda v: v[:, :4].contiguous(), "w scales must hold N\\*K/32"),
       "emax-dtype": ("emax", lambda v: v.int(), "stripe exponents must be uint8"),
       "emax-short": ("emax", lambda v: v[:4].contiguous(), "stripe exponents must hold K/32")}


@pytest.mark.parametrize("case", sorted(BAD))
def test_fused_mxfp4_gemm_dx_rejects(case):
    key, change, msg = BAD[case]
    a = dx_args()
    a[key] = change(a[key])
    with pytest.raises(RuntimeError, match=msg):
        ext().fused_mxfp4_gemm_dx(*a.values())
