"""The ragged-width fp8 kernels (`fused_fp8_gemm_ragged`, `quantize_rows_fp8_scaled_padded`,
`fused_fp8_gemm_dx_ragged`) and their dispatch, against float64, the CPU oracle of ops/quant.py
and the aligned kernels on zero-padded operands.  Helpers and bounds of test_gpu_fp8_gemm.py."""

import pytest
import torch
import torch.nn.functional as F

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

import relora_amd.ops.functional as Fn
from relora_amd.ops.quant import dequantize_fp8_ref, quantize_fp8_ref
from test_gpu_fp8_dx import BAD as BAD_DX, dx_args, dx_ref, misaligned
from test_gpu_fp8_gemm import (BAD as BAD_FWD, BF, F32, U, as_codes, assert_within, d, ext, gemm_args,
                               gen, poison, strided, ternary)

pytestmark = pytest.mark.gpu
EMPTY = torch.empty(0, dtype=BF, device="cuda")


def ceil_to(n, m):
    return (n + m - 1) // m * m


def rows_to(v, n):   # zero rows appended up to n
    return F.pad(v, (0, 0) * (v.dim() - 1) + (0, n - v.shape[0]))


@pytest.mark.parametrize("M,N,K,r,with_bias", [
    (256, N, K, r, b) for N in (1, 85, 264, 341, 511, 513) for K in (128, 384) for r in (0, 64, 128)
    for b in (False, True)] + [(512, 341, 128, 64, True), (256, 2133, 128, 64, True)])
def test_ragged_gemm_exact(M, N, K, r, with_bias):
    """The data of test_fused_fp8_gemm_exact: every partial sum is a small integer."""
    g = gen("ragged-exact", M, N, K, r, with_bias)
    xv, wv = ternary((M, K), g), ternary((N, K), g)
    sx, sw = (torch.exp2(torch.randint(0, 2, (n,), generator=g).double()) for n in (M, N))
    t, bw = 2 * ternary((M, r), g), ternary((N, r), g)
    bias = torch.randint(-8, 9, (N,), generator=g).double() if with_bias else torch.zeros(N)
    ref = (xv @ wv.t()) * sx[:, None] * sw[None, :] + bias + (0.5 * t) @ bw.t()
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    poison(M, N)
    y = ext().fused_fp8_gemm_ragged(
        as_codes(xv), (448 * sx).float().cuda(), as_codes(wv), (448 * sw).float().cuda(), N,
        t.to(BF).cuda() if r else EMPTY, bw.to(BF).cuda() if r else EMPTY,
        bias.to(BF).cuda() if with_bias else EMPTY, 0.5)
    bad = ~(d(y) == ref)
    assert y.shape == (M, N) and not bad.any(), f"wrong in columns {bad.any(0).nonzero().flatten().tolist()[:16]}"


@pytest.mark.parametrize("M,N,K,r", [(256, 85, 256, 64), (256, 341, 256, 64),      # and the aligned kernel
                                     (256, 341, 384, 128), (512, 5461, 128, 64)])
def test_ragged_gemm_random(M, N, K, r):
    g, s = gen("ragged-random", M, N, K, r), 0.25
    (xq, xs), (wq, ws) = (quantize_fp8_ref(torch.randn(n, K, generator=g).to(BF)) for n in (M, N))
    t, bw, bias = (torch.randn(*sh, generator=g).to(BF) for sh in ((M, r), (N, r), (N,)))
    xd, wd, ts = dequantize_fp8_ref(xq, xs).double(), dequantize_fp8_ref(wq, ws).double(), (t * s).double()
    ref = xd @ wd.t() + ts @ bw.double().t() + bias.double()
    S = xd.abs() @ wd.abs().t() + ts.abs() @ bw.double().abs().t() + bias.double().abs()
    y = ext().fused_fp8_gemm_ragged(xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(), N, t.cuda(), bw.cuda(),
                                    bias.cuda(), s)
    assert_within(y, ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(y, ext().fused_fp8_gemm_ragged(xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(), N,
                                                      t.cuda(), bw.cuda(), bias.cuda(), s))
    if K == 256:
        Nn = ceil_to(N, 256)
        ya = ext().fused_fp8_gemm(xq.cuda(), xs.cuda(), rows_to(wq, Nn).cuda(), rows_to(ws, Nn).cuda(), Nn,
                                  t.cuda(), rows_to(bw, Nn).cuda(), rows_to(bias, Nn).cuda(), s)
        assert torch.equal(y, ya[:, :N])


@pytest.mark.parametrize("N", [1, 15, 16, 17, 85, 341, 5461, 8200])
def test_quantize_rows_scaled_padded(N):
    g, M = gen("qpad", N), 3
    ws = (torch.rand(N, generator=g) + 0.5) * torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())
    dy = (torch.randn(M, N, generator=g) * torch.tensor([0.125, 0.0, 8.0])[:, None]).to(BF)   # row 1: zeros
    codes_ref, amax_ref = quantize_fp8_ref(dy, col_scale=ws)
    codes, amax = ext().quantize_rows_fp8_scaled_padded(dy.cuda(), ws.cuda())
    assert codes.shape == (M, ceil_to(N, 128)) and codes.dtype == torch.uint8
    assert torch.equal(amax.cpu().view(torch.int32), amax_ref.view(torch.int32))
    assert torch.equal(codes.cpu()[:, :N], codes_ref) and not codes.cpu()[:, N:].any()


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("N", [1, 85, 213, 341])
def test_ragged_dx(N, K):
    """Exact values on the data of test_dx_exact; the aligned kernel on W zero-padded to Np rows;
    NaN codes (0xFF) in the memory directly behind W's N rows must not reach the result."""
    M, Np = 256, ceil_to(N, 128)
    g = gen("ragged-dx", N, K)
    gv, wv = ternary((M, N), g), ternary((N, K), g)
    sg = torch.exp2(torch.randint(0, 2, (M,), generator=g).double())
    ref = (gv @ wv) * sg[:, None]
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    gq, gs, wq = as_codes(F.pad(gv, (0, Np - N))), (448 * sg).float().cuda(), as_codes(wv)
    poison(M, K)
    dx = ext().fused_fp8_gemm_dx_ragged(gq, gs, wq, N, K)
    bad = ~(d(dx) == ref)
    assert not bad.any(), f"wrong per tile: {bad.view(256, K // 256, 256).sum(dim=(0, 2)).tolist()}"
    assert torch.equal(dx, ext().fused_fp8_gemm_dx(gq, gs, rows_to(wq, Np), K))
    behind = torch.full((Np + 128, K), 0xFF, dtype=torch.uint8, device="cuda")
    behind[:N] = wq
    assert torch.equal(dx, ext().fused_fp8_gemm_dx_ragged(gq, gs, behind[:N], N, K))


def test_ragged_module(monkeypatch):
    """ReLoRaLinear(256 -> 341, fp8) at M = 256: y of the ragged arm within the kernel's bound on the
    operands it was handed; dx with the switch on within test_fp8_backward_switch's bound for the
    fused arm; with the switch off, and with RELORA_AMD_FP8_RAGGED=0, the materialize arm's dx."""
    from relora_amd.relora import ReLoRaLinear
    M, K, N, r, s = 256, 256, 341, 64, 0.25
    g = gen("ragged-module")
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize="fp8", bias=True,
                       weight_data=torch.randn(N, K, generator=g) * 0.05)
    with torch.no_grad():
        lin.lora_A.weight.copy_(torch.randn(r, K, generator=g) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(N, r, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.1)
    lin = lin.to(device="cuda", dtype=BF)
    x = torch.randn(M, K, generator=g).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(M, N, generator=g).to(BF).cuda()
    A, B, qw = lin.lora_A.weight, lin.lora_B.weight, lin.weight
    out = {}
    for arm, ragged, on in (("off", True, False), ("on", True, True), ("materialize", False, True)):
        monkeypatch.setattr(Fn, "_FP8_RAGGED", ragged)
        lin.fp8_backward, x.grad = on, None
        y = lin(x)
        y.backward(dy)
        out[arm] = (y.detach(), x.grad.clone())
    wq, ws = qw.qdata.cpu().view(N, K), qw.absmax.cpu()
    xf, Wf = dequantize_fp8_ref(*quantize_fp8_ref(x.detach().cpu())).double(), dequantize_fp8_ref(wq, ws).double()
    ts, B64, b64 = d((x.detach() @ A.t()) * s), d(B), d(lin.bias)   # t_u as the module computes it
    ref = xf @ Wf.t() + ts @ B64.t() + b64
    S = xf.abs() @ Wf.abs().t() + ts.abs() @ B64.abs().t() + b64.abs()
    assert_within(out["on"][0], ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(out["off"][0], out["on"][0]) and not torch.equal(out["on"][0], out["materialize"][0])
    A64, dy64 = d(A), d(dy)
    us, (_, _, main, S8) = dy64 @ (s * B64), dx_ref(dy.cpu(), wq, ws)
    lora = us @ A64
    assert_within(out["on"][1], main + lora, U * (main + lora).abs() + U * main.abs() + U * lora.abs()
                  + U * (us.abs() @ A64.abs()) + (N + r) * F32 * (S8 + dy64.abs() @ (s * B64).abs() @ A64.abs()), "dx")
    assert torch.equal(out["off"][1], out["materialize"][1]) and not torch.equal(out["on"][1], out["off"][1])


FWD = {k: v for k, v in BAD_FWD.items() if k != "N-128"}   # N = 128 is a shape of the ragged kernel
FWD.update({n + "-misaligned": (n, misaligned, "16-byte aligned") for n in ("xq", "wq")})
DX = dict(BAD_DX, **{"N-64": ("gq", lambda v: v[:, :64].contiguous(), "N rounded up to 128"),
                     "N-0": ("N", lambda v: 0, "must be > 0"), "N-129": ("N", lambda v: 129, "N rounded up to 128")})
QP = {"dy-cpu": ("dy", lambda v: v.cpu(), "dy must be a GPU tensor"), "dy-1d": ("dy", lambda v: v.view(-1), "dy must be 2-D"),
      "dy-strided": ("dy", strided, "dy must be contiguous"), "dy-dtype": ("dy", lambda v: v.float(), "dy must be bf16"),
      "dy-empty": ("dy", lambda v: v[:0], "must be > 0"), "ws-cpu": ("ws", lambda v: v.cpu(), "ws must be on dy's device"),
      "ws-dtype": ("ws", lambda v: v.double(), "ws must be fp32"), "ws-strided": ("ws", strided, "ws must be contiguous"),
      "ws-short": ("ws", lambda v: v[:16].contiguous(), "ws must hold one value")}
ENTRY = {"fused_fp8_gemm_ragged": (FWD, gemm_args), "fused_fp8_gemm_dx_ragged": (DX, lambda: dict(dx_args(), N=128)),
         "quantize_rows_fp8_scaled_padded": (QP, lambda: dict(dy=torch.zeros(4, 33, dtype=BF, device="cuda"),
                                                              ws=torch.ones(33, device="cuda")))}


@pytest.mark.parametrize("fn,case", [(fn, c) for fn, (bad, _) in ENTRY.items() for c in sorted(bad)])
def test_ragged_rejects(fn, case):
    (key, change, msg), a = ENTRY[fn][0][case], ENTRY[fn][1]()
    a[key] = change(a[key])
    if "dx" in fn:
        a = dict(gq=a["gq"], gs=a["gs"], wq=a["wq"], N=a["N"], K=a["K"])   # the entry point's order
    with pytest.raises(RuntimeError, match=msg):
        getattr(ext(), fn)(*a.values())
