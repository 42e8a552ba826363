"""`fused_mxfp4_gemm_ragged` (any N, any K) and its dispatch, against float64, ops/quant.py's reference
and the aligned kernel on padded operands.  Helpers and bounds of test_gpu_mxfp4_gemm.py."""

import pytest
import torch
import torch.nn.functional as F

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

import relora_amd.ops.functional as Fn
from relora_amd.ops.quant import dequantize_fp8_ref, dequantize_mxfp4_ref, quantize_fp8_ref, quantize_mxfp4_ref
from test_gpu_fp8_dx import misaligned
from test_gpu_fp8_gemm import poison
from test_gpu_mxfp4_gemm import BAD as BAD_ALIGNED, BF, F32, U, as_codes, assert_within, d, ext, gen, ternary

pytestmark = pytest.mark.gpu
EMPTY = torch.empty(0, dtype=BF, device="cuda")


def ceil_to(n, m):
    return (n + m - 1) // m * m


def grown(v, rows, cols, fill=0):   # v in the top left corner of [rows, cols]
    return F.pad(v, (0, cols - v.shape[1], 0, rows - v.shape[0]), value=fill)


def behind_ff(v, off):   # the same bytes `off` bytes into a buffer of 0xFF (NaN as E8M0)
    buf = torch.full((v.numel() + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[off:off + v.numel()] = v.flatten()
    return buf[off:off + v.numel()].view(v.shape)


ALL_N, ALL_K = (1, 85, 256, 264, 341, 513), (1, 31, 32, 33, 96, 128, 160, 341, 384)
SHAPES = ([(256, N, K) for N in (85, 256) for K in ALL_K] + [(256, N, K) for N in ALL_N for K in (128, 160)]
          + [(256, 341, 384), (512, 341, 160)])
EXACT = ([s + (r, b) for s in sorted(set(SHAPES)) for r in (0, 64, 128) for b in (False, True)]
         + [(256, 256, 5461, 64, True), (256, 5461, 128, 128, False)])


@pytest.mark.parametrize("M,N,K,r,with_bias", EXACT)
def test_ragged_gemm_exact(M, N, K, r, with_bias):
    """The data of test_fused_mxfp4_gemm_exact: every partial sum is a multiple of 2^-3 far below 2^21.
    The aligned kernel on operands padded with zero codes, scale byte 127 and zero bw / bias rows adds
    zeros only: the same bits.  0xFF around W's codes and scales must not reach the result."""
    g = gen("ragged-exact", M, N, K, r, with_bias)
    Kp, Ka, Np, bpr = ceil_to(K, 32), ceil_to(K, 128), ceil_to(N, 256), ceil_to(K, 32) // 32
    xv, sx = ternary((M, K), g), torch.exp2(torch.randint(0, 3, (M,), generator=g).double())
    nib = torch.randint(0, 16, (N, Kp), generator=g).to(torch.uint8)
    nib[:, K:] = 0   # the padding of a short last block is zero codes
    wq = nib[:, 0::2] | (nib[:, 1::2] << 4)
    ws = torch.randint(125, 130, (N, bpr), generator=g).to(torch.uint8)
    t, bw = 2 * ternary((M, r), g), ternary((N, r), g)
    bias = torch.randint(-8, 9, (N,), generator=g).double() if with_bias else torch.zeros(N)
    ref = (xv @ dequantize_mxfp4_ref(wq, ws, K).double().t()) * sx[:, None] + bias + (0.5 * t) @ bw.t()
    assert ref.abs().max() < 2 ** 21 and torch.equal(ref * 8, (ref * 8).round())
    xq, xs = as_codes(F.pad(xv, (0, Ka - K))), (448 * sx).float().cuda()
    tb, bwb, bb = t.to(BF).cuda() if r else EMPTY, bw.to(BF), bias.to(BF)
    tail = (tb, bwb.cuda() if r else EMPTY, bb.cuda() if with_bias else EMPTY, 0.5)
    poison(M, N)
    y = ext().fused_mxfp4_gemm_ragged(xq, xs, wq.cuda(), ws.cuda(), N, K, *tail)
    bad = ~(d(y) == ref.float().to(BF).double())
    assert y.shape == (M, N) and not bad.any(), f"wrong in columns {bad.any(0).nonzero().flatten().tolist()[:16]}"
    padded = ext().fused_mxfp4_gemm(xq, xs, grown(wq, Np, Ka // 2).cuda(), grown(ws, Np, Ka // 32, 127).cuda(), Np, tb,
                                    grown(bwb, Np, r).cuda() if r else EMPTY,
                                    F.pad(bb, (0, Np - N)).cuda() if with_bias else EMPTY, 0.5)
    assert torch.equal(y, padded[:, :N])
    off = 4 if N == Np and K == Ka else 1   # aligned shapes run the aligned kernel: whole scale dwords
    assert torch.equal(y, ext().fused_mxfp4_gemm_ragged(xq, xs, behind_ff(wq, 16), behind_ff(ws, off), N, K, *tail))


@pytest.mark.parametrize("s", [0.25, 1.0])
@pytest.mark.parametrize("M,N,K,r", [(256, 341, 352, 128), (512, 85, 5461, 64), (256, 5461, 384, 64)])
def test_ragged_gemm_random(M, N, K, r, s):
    g = gen("ragged-random", M, N, K, r, s)
    xq, xs = quantize_fp8_ref(torch.randn(M, K, generator=g).to(BF))
    wq, ws = quantize_mxfp4_ref(torch.randn(N, K, generator=g).to(BF))
    t, bw, bias = (torch.randn(*sh, generator=g).to(BF) for sh in ((M, r), (N, r), (N,)))
    xd, wd, ts = dequantize_fp8_ref(xq, xs).double(), dequantize_mxfp4_ref(wq, ws, K).double(), (t * s).double()
    ref = xd @ wd.t() + ts @ bw.double().t() + bias.double()
    S = xd.abs() @ wd.abs().t() + ts.abs() @ bw.double().abs().t() + bias.double().abs()
    args = (F.pad(xq, (0, ceil_to(K, 128) - K)).cuda(), xs.cuda(), wq.cuda(), ws.cuda(), N, K, t.cuda(), bw.cuda(),
            bias.cuda(), s)
    y = ext().fused_mxfp4_gemm_ragged(*args)
    assert_within(y, ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(y, ext().fused_mxfp4_gemm_ragged(*args))


@pytest.mark.parametrize("K,N", [(256, 341), (341, 256)])
def test_ragged_module(K, N, monkeypatch):
    """ReLoRaLinear at M = 256 with the switch on and off; the bounds of
    test_mxfp4_relora_linear_fwd_bwd_merge, `fused` following the switch."""
    from relora_amd.relora import ReLoRaLinear
    M, r, s = 256, 64, 0.25
    g = gen("ragged-module", K, N)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="mxfp4", bias=True,
                       weight_data=torch.randn(N, K, generator=g) * 0.05)
    with torch.no_grad():
        lin.lora_A.weight.copy_(torch.randn(r, K, generator=g) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(N, r, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.1)
    lin = lin.to(device="cuda", dtype=BF)
    x = torch.randn(M, K, generator=g).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(M, N, generator=g).to(BF).cuda()
    A, B, qw = lin.lora_A.weight, lin.lora_B.weight, lin.weight
    Wb = qw.materialize(BF)
    x64, A64, B64 = (d(v).requires_grad_(True) for v in (x, A, B))
    W64, b64, dy64 = d(Wb), d(lin.bias), d(dy)
    (x64 @ W64.t() + b64 + (s * (x64 @ A64.t())) @ B64.t()).backward(dy64)
    xa, Aa, sBa, Wa, dya = (v.detach().abs() for v in (x64, A64, s * B64, W64, dy64))
    t, us = (x64 @ A64.t()).detach(), dy64 @ (s * B64).detach()
    xA, dysB, lora = xa @ Aa.t(), dya @ sBa, (s * t) @ B64.detach().t()
    ys = {}
    for fused in (True, False):
        monkeypatch.setattr(Fn, "_MXFP4_RAGGED", fused)
        x.grad = A.grad = B.grad = None
        y = lin(x)
        y.backward(dy)
        ys[fused] = y.detach()
        xf = dequantize_fp8_ref(*quantize_fp8_ref(x.detach().cpu())).double() if fused else x64.detach()
        main = xf @ W64.t() + b64
        by = (U * (main + lora).abs() + U * (t.abs() @ sBa.t())
              + (K + r) * F32 * (xf.abs() @ Wa.t() + xA @ sBa.t() + b64.abs()))
        if not fused:   # F.linear and lora_add_nt_ round their products to bf16
            by = by + U * main.abs() + U * lora.abs()
        assert_within(y, main + lora, by, f"y fused={fused}")
        bdx = (U * x64.grad.abs() + U * (dy64 @ W64).abs() + U * (us @ A64.detach()).abs()
               + U * (us.abs() @ Aa) + (N + r) * F32 * (dya @ Wa + dysB @ Aa))
        assert_within(x.grad, x64.grad, bdx, "dx")
        assert_within(A.grad, A64.grad, U * A64.grad.abs() + U * (us.abs().t() @ xa)
                      + (M + N) * F32 * (dysB.t() @ xa), "dA")
        assert_within(B.grad, B64.grad, U * B64.grad.abs() + U * s * (dya.t() @ t.abs())
                      + (M + K) * F32 * s * (dya.t() @ xA), "dB")
    assert not torch.equal(ys[True], ys[False])
    with torch.no_grad():
        merged = Wb + B @ A * s
    lin.merge_and_reinit()
    codes, scales = quantize_mxfp4_ref(merged.cpu())
    assert torch.equal(qw.qdata.cpu(), codes) and torch.equal(qw.absmax.cpu(), scales)


def ragged_args():   # N = 341, K = 40: two blocks a row
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    return dict(xq=z(256, 128, dt=torch.uint8), xs=z(256, dt=torch.float32), wq=z(341, 32, dt=torch.uint8),
                ws=z(341, 2, dt=torch.uint8), N=341, K=40, t=z(256, 64), bw=z(341, 64), bias=z(341), scale=0.5)


BAD = {k: v for k, v in BAD_ALIGNED.items() if k not in ("K-64", "N-128", "wq-short", "ws-short", "ws-offset")}
BAD.update({"xq-wide": ("xq", lambda v: v.new_zeros(256, 256), "K rounded up to 128"),
            "K-129": ("K", lambda v: 129, "K rounded up to 128"), "K-0": ("K", lambda v: 0, "must be > 0"),
            "K-2^24": ("K", lambda v: 1 << 24, "shape too large"),
            "K-72": ("K", lambda v: 72, r"w codes must hold N\*Kp/2"),
            "wq-short": ("wq", lambda v: v[:340].contiguous(), r"w codes must hold N\*Kp/2"),
            "ws-short": ("ws", lambda v: v[:, :1].contiguous(), r"w scales must hold N\*ceil\(K/32\)"),
            "N-340": ("N", lambda v: 340, "w codes must hold"),
            "xq-misaligned": ("xq", misaligned, "x codes must be 16-byte aligned"),
            "wq-misaligned": ("wq", misaligned, "w codes must be 16-byte aligned")})


@pytest.mark.parametrize("case", sorted(BAD))
def test_ragged_gemm_rejects(case):
    key, change, msg = BAD[case]
    a = ragged_args()
    a[key] = change(a[key])
    with pytest.raises(RuntimeError, match=msg):
        ext().fused_mxfp4_gemm_ragged(*a.values())
