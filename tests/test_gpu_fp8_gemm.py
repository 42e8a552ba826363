"""fp8_gemm.hip and `ReLoRaLinear(quantize="fp8")` against the CPU oracle of
ops/quant.py and float64.  Bounds as test_gpu_fused_gemm.py derives them: 2^-8
per bf16 rounding, n * 2^-23 * sum|a_i b_i| per fp32 dot product of length n."""

import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd.ops import hip
from relora_amd.ops.quant import dequantize_fp8_ref, quantize_fp8_ref

BF, E4, U, F32 = torch.bfloat16, torch.float8_e4m3fn, 2.0 ** -8, 2.0 ** -23
ext = hip.ext_or_raise


def d(t):
    return t.detach().cpu().double()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def assert_within(got, ref, bound, what):
    ratio = (d(got) - ref).abs() / bound.clamp_min(1e-300)
    assert bool((ratio <= 1).all()), f"{what}: {int((ratio > 1).sum())} past the bound, worst {ratio.max():.3f}x"


# ties (17 -> 16, 19 -> 20, 2^-10 -> 0, 3*2^-10 -> 2^-8), subnormals, -0
SPECIAL = [17.0, -19.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, -5 * 2.0 ** -9, -0.0]


@pytest.mark.parametrize("K", [16, 128, 208, 4096,   # lane group; wave, 4 units a lane
                               528, 2000, 8176,      # wave with 1, 2, 8 units a lane
                               8208, 100])           # looping form; scalar form
@pytest.mark.parametrize("R", [1, 5, 64])
def test_quantize_and_dequantize_rows(R, K):
    """+-448 * 2^e_r once a row, smaller bf16 values elsewhere: inv = 2^-e_r, v * inv exact."""
    g = gen("q", R, K)
    x = (torch.randn(R, K, generator=g) * 100).clamp(-440, 440).to(BF).float()
    x[:, 1:8] = torch.tensor(SPECIAL)
    x[torch.arange(R), (torch.arange(R) * 7) % K] = 448.0 * (1 - 2 * (torch.arange(R) % 2))
    x = x * torch.exp2((torch.arange(R) % 9 - 4).float()).unsqueeze(1)
    x[3:4] = 0   # a row of zeros wherever there is a row 3
    x = x.to(BF)
    codes_ref, amax_ref = quantize_fp8_ref(x)
    codes, amax = ext().quantize_rows_fp8(x.cuda())
    assert torch.equal(amax.cpu().view(torch.int32), amax_ref.view(torch.int32))
    got, want = codes.cpu().view(E4).float(), codes_ref.view(E4).float()
    assert want.abs().max() == 448 and bool((got == want).all())
    # random rows: 24-bit products, inv from a correctly rounded division on both sides
    xr = torch.randn(R, K, generator=g).to(BF)
    got, want = ext().quantize_rows_fp8(xr.cuda())[0].cpu(), quantize_fp8_ref(xr)[0]
    assert bool((got.view(E4).float() == want.view(E4).float()).all())
    for dtype in (BF, torch.float32):
        back = ext().dequantize_rows_fp8(codes, amax, R, K, dtype)
        assert torch.equal(back.cpu(), dequantize_fp8_ref(codes.cpu(), amax.cpu(), dtype))


def ternary(shape, g, density=0.25):
    u = torch.rand(shape, generator=g)
    return (u < density / 2).double() - (u > 1 - density / 2).double()


def as_codes(v):
    return v.float().to(E4).view(torch.uint8).cuda()


def poison(M, N):  # NaN in the block the allocator most likely reuses for the output
    torch.full((M, N), float("nan"), dtype=BF, device="cuda")


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("r", [0, 64, 256])
@pytest.mark.parametrize("K", [128, 256, 384, 640])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 256), (256, 768), (768, 768)])
def test_fused_fp8_gemm_exact(M, N, K, r, with_bias):
    """Ternary codes, power-of-two scales, t = 2 * ternary at 0.5, integer bias: all sums exact."""
    g = gen("exact", M, N, K, r, with_bias)
    xv, wv = ternary((M, K), g), ternary((N, K), g)
    sx, sw = (torch.exp2(torch.randint(0, 2, (n,), generator=g).double()) for n in (M, N))
    t, bw = 2 * ternary((M, r), g), ternary((N, r), g)
    bias = torch.randint(-8, 9, (N,), generator=g).double() if with_bias else torch.zeros(N)
    ref = (xv @ wv.t()) * sx[:, None] * sw[None, :] + bias + (0.5 * t) @ bw.t()
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    empty = torch.empty(0, dtype=BF, device="cuda")
    poison(M, N)
    y = ext().fused_fp8_gemm(
        as_codes(xv), (448 * sx).float().cuda(), as_codes(wv), (448 * sw).float().cuda(), N,
        t.to(BF).cuda() if r else empty, bw.to(BF).cuda() if r else empty,
        bias.to(BF).cuda() if with_bias else empty, 0.5)
    bad = ~(d(y) == ref)
    assert not bad.any(), f"wrong per tile: {bad.view(M // 256, 256, N // 256, 256).sum(dim=(1, 3)).tolist()}"


@pytest.mark.parametrize("s", [0.25, 1.0])
@pytest.mark.parametrize("M,N,K,r", [(768, 768, 384, 128), (512, 1024, 640, 192)])
def test_fused_fp8_gemm_random(M, N, K, r, s):
    g = gen("random", M, N, K, r, s)
    (xq, xs), (wq, ws) = (quantize_fp8_ref(torch.randn(n, K, generator=g).to(BF)) for n in (M, N))
    t, bw, bias = (torch.randn(*sh, generator=g).to(BF) for sh in ((M, r), (N, r), (N,)))
    xd, wd = dequantize_fp8_ref(xq, xs).double(), dequantize_fp8_ref(wq, ws).double()
    ts = (t * s).double()     # the bf16 product the host hands to the kernel
    ref = xd @ wd.t() + ts @ bw.double().t() + bias.double()
    S = xd.abs() @ wd.abs().t() + ts.abs() @ bw.double().abs().t() + bias.double().abs()
    args = [v.cuda() for v in (xq, xs, wq, ws)] + [N, t.cuda(), bw.cuda(), bias.cuda(), s]
    y = ext().fused_fp8_gemm(*args)
    assert_within(y, ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(y, ext().fused_fp8_gemm(*args))


@pytest.mark.parametrize("M", [256, 200], ids=["fused", "materialize"])
def test_fp8_relora_linear_fwd_bwd_merge(M):
    """M = 256: fused fp8 arm; M = 200: materialize arm.  Backward on bf16 x and W; the merge."""
    from relora_amd.relora import ReLoRaLinear
    K, N, r, s = 256, 256, 64, 0.25
    g = gen("module", M)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="fp8",
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
    Wb, fused = qw.materialize(BF), M % 256 == 0
    x64, A64, B64 = (d(v).requires_grad_(True) for v in (x, A, B))
    W64, b64, dy64 = d(Wb), d(lin.bias), d(dy)
    (x64 @ W64.t() + b64 + (s * (x64 @ A64.t())) @ B64.t()).backward(dy64)
    xa, Aa, sBa, Wa, dya = (v.detach().abs() for v in (x64, A64, s * B64, W64, dy64))
    t, us = (x64 @ A64.t()).detach(), dy64 @ (s * B64).detach()
    xA, dysB = xa @ Aa.t(), dya @ sBa
    # y: the fused arm multiplies the fake-quantised x with the fp32 dequantised W
    xf = dequantize_fp8_ref(*quantize_fp8_ref(x.detach().cpu())).double() if fused else x64.detach()
    Wf = dequantize_fp8_ref(qw.qdata.cpu().view(N, K), qw.absmax.cpu()).double() if fused else W64
    main = xf @ Wf.t() + b64
    lora = (s * t) @ B64.detach().t()
    by = (U * (main + lora).abs() + U * (t.abs() @ sBa.t())
          + (K + r) * F32 * (xf.abs() @ Wf.abs().t() + xA @ sBa.t() + b64.abs()))
    if not fused:   # F.linear and lora_add_nt_ round their products to bf16
        by = by + U * main.abs() + U * lora.abs()
    assert_within(y, main + lora, by, "y")
    # dx, dA, dB: the terms of test_quantized_relora_linear_fwd_bwd_against_float64
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
    want = dequantize_fp8_ref(*quantize_fp8_ref(merged.cpu()), BF)
    assert torch.equal(lin.weight.materialize(BF).cpu(), want)


def gemm_args():
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return dict(xq=z(256, 128, dt=torch.uint8), xs=z(256, dt=torch.float32),
                wq=z(256, 128, dt=torch.uint8), ws=z(256, dt=torch.float32), N=256,
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
       "wq-short": ("wq", lambda v: v[:128].contiguous(), "w codes must hold"),
       "xs-short": ("xs", lambda v: v[:128].contiguous(), "x absmax must hold one value"),
       "ws-short": ("ws", lambda v: v[:128].contiguous(), "w absmax must hold one value")}
for _n, _what in [("xq", "x codes"), ("wq", "w codes"), ("xs", "x absmax"), ("ws", "w absmax"),
                  ("t", "t"), ("bw", "bw"), ("bias", "bias")]:
    if _n != "xq":
        BAD[_n + "-cpu"] = (_n, lambda v: v.cpu(), _what + " must be on xq's")
    BAD[_n + "-strided"] = (_n, strided, _what + " must be contiguous")
    BAD[_n + "-dtype"] = (_n, lambda v: v.to(torch.float16), _what + " must be "
                           + ("uint8" if "codes" in _what else "fp32" if "absmax" in _what else "bf16"))


@pytest.mark.parametrize("case", sorted(BAD))
def test_fused_fp8_gemm_rejects(case):
    key, change, msg = BAD[case]
    a = gemm_args()
    a[key] = change(a[key])
    with pytest.raises(RuntimeError, match=msg):
        ext().fused_fp8_gemm(*a.values())


@pytest.mark.parametrize("fn,args,msg", [
    ("quantize_rows_fp8", lambda x, q, a: (x.cpu(),), "x must be a GPU tensor"),
    ("quantize_rows_fp8", lambda x, q, a: (x.view(-1),), "x must be 2-D"),
    ("quantize_rows_fp8", lambda x, q, a: (strided(x),), "x must be contiguous"),
    ("quantize_rows_fp8", lambda x, q, a: (x.float(),), "x must be bf16"),
    ("quantize_rows_fp8", lambda x, q, a: (x[:0],), "R and K must be > 0"),
    ("dequantize_rows_fp8", lambda x, q, a: (q.cpu(), a, 4, 32, BF), "codes must be a GPU tensor"),
    ("dequantize_rows_fp8", lambda x, q, a: (q.to(torch.int8), a, 4, 32, BF), "contiguous uint8"),
    ("dequantize_rows_fp8", lambda x, q, a: (q, a, 4, 16, BF), "codes must hold"),
    ("dequantize_rows_fp8", lambda x, q, a: (q, a[:2], 4, 32, BF), "absmax must be R"),
    ("dequantize_rows_fp8", lambda x, q, a: (q, a, 4, 32, torch.float16), "bf16 or fp32")])
def test_row_quantiser_rejects(fn, args, msg):
    x = torch.zeros(4, 32, dtype=BF, device="cuda")
    q, a = torch.zeros(4, 32, dtype=torch.uint8, device="cuda"), torch.ones(4, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        getattr(ext(), fn)(*args(x, q, a))
