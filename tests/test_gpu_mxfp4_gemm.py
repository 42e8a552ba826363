"""mxfp4_gemm.hip and `ReLoRaLinear(quantize="mxfp4")` against ops/quant.py's reference and float64.
Bounds as test_gpu_fp8_gemm.py: 2^-8 per bf16 rounding, n * 2^-23 * sum|a_i b_i| per fp32 dot product."""

import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from test_mxfp4_quant import hand_rows

from relora_amd.ops import hip
from relora_amd.ops.quant import (dequantize_fp8_ref, dequantize_mxfp4_ref, quantize_fp8_ref,
                                  quantize_mxfp4_ref)

BF, E4, U, F32 = torch.bfloat16, torch.float8_e4m3fn, 2.0 ** -8, 2.0 ** -23
ext = hip.ext_or_raise


def d(t):
    return t.detach().cpu().double()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def assert_within(got, ref, bound, what):
    ratio = (d(got) - ref).abs() / bound.clamp_min(1e-300)
    assert bool((ratio <= 1).all()), f"{what}: {int((ratio > 1).sum())} past the bound, worst {ratio.max():.3f}x"


@pytest.mark.parametrize("R,K", [(R, K) for R in (1, 3, 300) for K in (32, 64, 160, 53)]
                         + [(3, 5461), ("hand", 64), ("hand", 53)])
def test_quantize_and_dequantize_rows(R, K):
    """Vector kernel (K % 32 == 0) and scalar arm, bit-equal to the reference both ways."""
    if R == "hand":
        x = hand_rows()[0][:, :K].contiguous().to(BF)
    else:   # normal data, the scale of a row moving over 2^-6 .. 2^6, a block of zeros
        x = torch.randn(R, K, generator=gen("q", R, K)) * torch.exp2(torch.arange(R) % 13 - 6.0)[:, None]
        x[R // 2, :32] = 0
        x = x.to(BF)
    codes_ref, scales_ref = quantize_mxfp4_ref(x)
    codes, scales = ext().quantize_rows_mxfp4(x.cuda())
    assert torch.equal(scales.cpu(), scales_ref) and torch.equal(codes.cpu(), codes_ref)
    for dtype in (BF, torch.float32):
        back = ext().dequantize_rows_mxfp4(codes, scales, x.shape[0], K, dtype)
        want = dequantize_mxfp4_ref(codes_ref, scales_ref, K, dtype)
        assert torch.equal(back.cpu().view(torch.uint8), want.view(torch.uint8))   # bit-equal


def ternary(shape, g, density=0.25):
    u = torch.rand(shape, generator=g)
    return (u < density / 2).double() - (u > 1 - density / 2).double()


def as_codes(v):
    return v.float().to(E4).view(torch.uint8).cuda()


EMPTY = dict(dtype=BF, device="cuda")


def test_staged_image_read_back():
    """x = I: y[m, n] is W[n, m] as the matrix core decoded it.  Every code in every nibble
    of a dword, a different scale byte in each of a row's 8 blocks and in each row."""
    n, k = torch.arange(256)[:, None], torch.arange(256)[None, :]
    nib = ((k // 8 + k + n) % 16).to(torch.uint8).view(256, 128, 2)
    codes = nib[..., 0] | (nib[..., 1] << 4)
    scales = (119 + (k[:, :8] + n) % 16).to(torch.uint8)
    empty = torch.empty(0, **EMPTY)
    y = ext().fused_mxfp4_gemm(as_codes(torch.eye(256)), torch.full((256,), 448.0, device="cuda"),
                               codes.cuda(), scales.cuda(), 256, empty, empty, empty, 1.0)
    bad = d(y) != dequantize_mxfp4_ref(codes, scales, 256).t().double()
    assert not bad.any(), f"{int(bad.sum())} wrong, first at (m, n) = {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("r", [0, 64, 128])
@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 256), (256, 512), (768, 768)])
def test_fused_mxfp4_gemm_exact(M, N, K, r, with_bias):
    """Every partial sum is a multiple of 2^-3 far below 2^21: fp32 accumulation is exact."""
    g = gen("exact", M, N, K, r, with_bias)
    xv, sx = ternary((M, K), g), torch.exp2(torch.randint(0, 3, (M,), generator=g).double())
    wq = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    ws = torch.randint(125, 130, (N, K // 32), generator=g).to(torch.uint8)
    t, bw = 2 * ternary((M, r), g), ternary((N, r), g)
    bias = torch.randint(-8, 9, (N,), generator=g).double() if with_bias else torch.zeros(N)
    ref = (xv @ dequantize_mxfp4_ref(wq, ws, K).double().t()) * sx[:, None] + bias + (0.5 * t) @ bw.t()
    assert ref.abs().max() < 2 ** 21 and torch.equal(ref * 8, (ref * 8).round())
    empty = torch.empty(0, **EMPTY)
    torch.full((M, N), float("nan"), **EMPTY)   # NaN in the block the output most likely reuses
    y = ext().fused_mxfp4_gemm(
        as_codes(xv), (448 * sx).float().cuda(), wq.cuda(), ws.cuda(), N,
        t.to(BF).cuda() if r else empty, bw.to(BF).cuda() if r else empty,
        bias.to(BF).cuda() if with_bias else empty, 0.5)
    bad = ~(d(y) == ref.float().to(BF).double())
    assert not bad.any(), f"wrong per tile: {bad.view(M // 256, 256, N // 256, 256).sum(dim=(1, 3)).tolist()}"


@pytest.mark.parametrize("s", [0.25, 1.0])
@pytest.mark.parametrize("M,N,K,r", [(768, 768, 384, 128), (256, 1024, 640, 192)])
def test_fused_mxfp4_gemm_random(M, N, K, r, s):
    g = gen("random", M, N, K, r, s)
    xq, xs = quantize_fp8_ref(torch.randn(M, K, generator=g).to(BF))
    wq, ws = quantize_mxfp4_ref(torch.randn(N, K, generator=g).to(BF))
    t, bw, bias = (torch.randn(*sh, generator=g).to(BF) for sh in ((M, r), (N, r), (N,)))
    xd, wd = dequantize_fp8_ref(xq, xs).double(), dequantize_mxfp4_ref(wq, ws, K).double()
    ts = (t * s).double()     # the bf16 product the host hands to the kernel
    ref = xd @ wd.t() + ts @ bw.double().t() + bias.double()
    S = xd.abs() @ wd.abs().t() + ts.abs() @ bw.double().abs().t() + bias.double().abs()
    args = [v.cuda() for v in (xq, xs, wq, ws)] + [N, t.cuda(), bw.cuda(), bias.cuda(), s]
    y = ext().fused_mxfp4_gemm(*args)
    assert_within(y, ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(y, ext().fused_mxfp4_gemm(*args))


@pytest.mark.parametrize("M,K", [(256, 256), (200, 256), (256, 8320)], ids=["fused", "materialize", "long-K"])
def test_mxfp4_relora_linear_fwd_bwd_merge(M, K):
    """M = 256: fused arm; M = 200 or K > 8192: materialize arm.  Backward on bf16 x and
    W; the merge.  Bounds term by term as test_fp8_relora_linear_fwd_bwd_merge."""
    from relora_amd.relora import ReLoRaLinear
    N, r, s = 256, 64, 0.25
    g = gen("module", M, K)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="mxfp4",
                       bias=True, weight_data=torch.randn(N, K, generator=g) * 0.05)
    with torch.no_grad():
        lin.lora_A.weight.copy_(torch.randn(r, K, generator=g) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(N, r, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.1)
    lin = lin.to(device="cuda", dtype=BF)
    x = torch.randn(M, K, generator=g).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(M, N, generator=g).to(BF).cuda()
    y = lin(x)
    y.backward(dy)
    A, B, qw = lin.lora_A.weight, lin.lora_B.weight, lin.weight
    Wb, fused = qw.materialize(BF), M % 256 == 0 and K <= 8192
    x64, A64, B64 = (d(v).requires_grad_(True) for v in (x, A, B))
    W64, b64, dy64 = d(Wb), d(lin.bias), d(dy)   # MXFP4 values are exact in bf16
    (x64 @ W64.t() + b64 + (s * (x64 @ A64.t())) @ B64.t()).backward(dy64)
    xa, Aa, sBa, Wa, dya = (v.detach().abs() for v in (x64, A64, s * B64, W64, dy64))
    t, us = (x64 @ A64.t()).detach(), dy64 @ (s * B64).detach()
    xA, dysB = xa @ Aa.t(), dya @ sBa
    # y: the fused arm multiplies the fake-quantised x
    xf = dequantize_fp8_ref(*quantize_fp8_ref(x.detach().cpu())).double() if fused else x64.detach()
    main = xf @ W64.t() + b64
    lora = (s * t) @ B64.detach().t()
    by = (U * (main + lora).abs() + U * (t.abs() @ sBa.t())
          + (K + r) * F32 * (xf.abs() @ Wa.t() + xA @ sBa.t() + b64.abs()))
    if not fused:   # F.linear and lora_add_nt_ round their products to bf16
        by = by + U * main.abs() + U * lora.abs()
    assert_within(y, main + lora, by, "y")
    bdx = (U * x64.grad.abs() + U * (dy64 @ W64).abs() + U * (us @ A64.detach()).abs()
           + U * (us.abs() @ Aa) + (N + r) * F32 * (dya @ Wa + dysB @ Aa))
    assert_within(x.grad, x64.grad, bdx, "dx")
    assert_within(A.grad, A64.grad, U * A64.grad.abs() + U * (us.abs().t() @ xa)
                  + (M + N) * F32 * (dysB.t() @ xa), "dA")
    assert_within(B.grad, B64.grad, U * B64.grad.abs() + U * s * (dya.t() @ t.abs())
                  + (M + K) * F32 * s * (dya.t() @ xA), "dB")
    with torch.no_grad():
        merged = Wb + B @ A * s
    lin.merge_and_reinit()
    codes, scales = quantize_mxfp4_ref(merged.cpu())
    assert torch.equal(qw.qdata.cpu(), codes) and torch.equal(qw.absmax.cpu(), scales)


def gemm_args():
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return dict(xq=z(256, 128, dt=torch.uint8), xs=z(256, dt=torch.float32),
                wq=z(256, 64, dt=torch.uint8), ws=z(256, 4, dt=torch.uint8), N=256,
                t=z(256, 64), bw=z(256, 64), bias=z(256), scale=0.5)


def strided(t):
    return torch.zeros(*t.shape[:-1], t.shape[-1] * 2, dtype=t.dtype, device=t.device)[..., ::2]


BAD = {"xq-cpu": ("xq", lambda v: v.cpu(), "xq must be a GPU tensor"),
       "xq-1d": ("xq", lambda v: v.view(-1), "xq must be 2-D"),
       "M-128": ("xq", lambda v: v[:128].contiguous(), "requires M%256==0"),
       "K-64": ("xq", lambda v: v[:, :64].contiguous(), "requires M%256==0"),
       "N-128": ("N", lambda v: 128, "requires M%256==0"),
       "N-0": ("N", lambda v: 0, "must be > 0"),
       "r-48": ("t", lambda v: v[:, :48].contiguous(), "r must be a multiple"),
       "r-320": ("t", lambda v: v.new_zeros(256, 320), "r must be a multiple"),
       "t-rows": ("t", lambda v: v[:128].contiguous(), r"t must be \[M, r\]"),
       "bw-rows": ("bw", lambda v: v[:128].contiguous(), r"bw must be \[N, r\]"),
       "bw-rank": ("bw", lambda v: v[:, :32].contiguous(), r"bw must be \[N, r\]"),
       "bias-short": ("bias", lambda v: v[:128].contiguous(), "bias must have N elements"),
       "wq-short": ("wq", lambda v: v[:128].contiguous(), r"w codes must hold N\*K/2"),
       "ws-short": ("ws", lambda v: v[:, :2].contiguous(), r"w scales must hold N\*K/32"),
       "ws-offset": ("ws", lambda v: v.new_zeros(1040)[1:1025], "w scales must be 16-byte aligned"),
       "xs-short": ("xs", lambda v: v[:128].contiguous(), "x absmax must hold one value")}
for _n, _what, _dt in [("xq", "x codes", "uint8"), ("wq", "w codes", "uint8"), ("ws", "w scales", "uint8"),
                       ("xs", "x absmax", "fp32"), ("t", "t", "bf16"), ("bw", "bw", "bf16"),
                       ("bias", "bias", "bf16")]:
    if _n != "xq":
        BAD[_n + "-cpu"] = (_n, lambda v: v.cpu(), _what + " must be on xq's")
    BAD[_n + "-strided"] = (_n, strided, _what + " must be contiguous")
    BAD[_n + "-dtype"] = (_n, lambda v: v.to(torch.float16), f"{_what} must be {_dt}")


@pytest.mark.parametrize("case", sorted(BAD))
def test_fused_mxfp4_gemm_rejects(case):
    key, change, msg = BAD[case]
    a = gemm_args()
    a[key] = change(a[key])
    with pytest.raises(RuntimeError, match=msg):
        ext().fused_mxfp4_gemm(*a.values())

