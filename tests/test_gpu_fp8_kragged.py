"""The fp8 kernels for a ragged reduction width (`quantize_rows_fp8_padded`, `fused_fp8_gemm_kragged`,
`fused_fp8_gemm_dx_kragged`) and their dispatch, against float64, the CPU oracle of ops/quant.py and
the ragged-N kernels on zero-padded operands.  Helpers and bounds of test_gpu_fp8_gemm.py."""

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


def cols_to(v, k):   # zero columns appended up to k
    return F.pad(v, (0, k - v.shape[1]))


def behind_ff(wq):   # the same codes at an odd address, NaN codes (0xFF) before and behind them
    buf = torch.full((wq.numel() + 513,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[1:1 + wq.numel()] = wq.flatten()
    return buf[1:1 + wq.numel()].view(wq.shape)


@pytest.mark.parametrize("K", [1, 15, 17, 127, 129, 341, 5461, 8200])
def test_quantize_rows_padded(K):
    g, M = gen("qkpad", K), 3
    x = (torch.randn(M, K, generator=g) * torch.tensor([0.125, 0.0, 8.0])[:, None]).to(BF)   # row 1: zeros
    codes_ref, amax_ref = quantize_fp8_ref(x)
    codes, amax = ext().quantize_rows_fp8_padded(x.cuda())
    assert codes.shape == (M, ceil_to(K, 128)) and codes.dtype == torch.uint8
    assert torch.equal(amax.cpu().view(torch.int32), amax_ref.view(torch.int32))
    assert torch.equal(codes.cpu()[:, :K], codes_ref) and not codes.cpu()[:, K:].any()


# tail-only tiles (7: shorter than a chunk), 1- and 127-byte tails, both buffer parities, row pitches
# that are odd, 2 mod 4, 4 mod 16 and 16 mod 128
@pytest.mark.parametrize("N,K,r,with_bias", [(N, K, r, b) for K in (7, 85, 129, 130, 132, 144, 255, 341, 389)
                                             for N in (256, 341) for r in (0, 64) for b in (False, True)])
def test_kragged_gemm_exact(N, K, r, with_bias):
    """The data of test_ragged_gemm_exact: every partial sum is a small integer.  The ragged-N kernel
    on both operands zero-padded to Kp columns adds zero codes only: the same bits."""
    M, Kp = 256, ceil_to(K, 128)
    g = gen("kragged-exact", N, K, r, with_bias)
    xv, wv = ternary((M, K), g), ternary((N, K), g)
    sx, sw = (torch.exp2(torch.randint(0, 2, (n,), generator=g).double()) for n in (M, N))
    t, bw = 2 * ternary((M, r), g), ternary((N, r), g)
    bias = torch.randint(-8, 9, (N,), generator=g).double() if with_bias else torch.zeros(N)
    ref = (xv @ wv.t()) * sx[:, None] * sw[None, :] + bias + (0.5 * t) @ bw.t()
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    xq, xs, wq, ws = as_codes(cols_to(xv, Kp)), (448 * sx).float().cuda(), as_codes(wv), (448 * sw).float().cuda()
    tail = (t.to(BF).cuda() if r else EMPTY, bw.to(BF).cuda() if r else EMPTY,
            bias.to(BF).cuda() if with_bias else EMPTY, 0.5)
    poison(M, N)
    y = ext().fused_fp8_gemm_kragged(xq, xs, wq, ws, N, K, *tail)
    bad = ~(d(y) == ref)
    assert y.shape == (M, N) and not bad.any(), f"wrong in columns {bad.any(0).nonzero().flatten().tolist()[:16]}"
    assert torch.equal(y, ext().fused_fp8_gemm_ragged(xq, xs, as_codes(cols_to(wv, Kp)), ws, N, *tail))
    assert torch.equal(y, ext().fused_fp8_gemm_kragged(xq, xs, behind_ff(wq), ws, N, K, *tail))


@pytest.mark.parametrize("M,N,K,r", [(256, 341, 341, 64), (512, 256, 5461, 64)])
def test_kragged_gemm_random(M, N, K, r):
    g, s = gen("kragged-random", M, N, K, r), 0.25
    (xq, xs), (wq, ws) = (quantize_fp8_ref(torch.randn(n, K, generator=g).to(BF)) for n in (M, N))
    t, bw, bias = (torch.randn(*sh, generator=g).to(BF) for sh in ((M, r), (N, r), (N,)))
    xd, wd, ts = dequantize_fp8_ref(xq, xs).double(), dequantize_fp8_ref(wq, ws).double(), (t * s).double()
    ref = xd @ wd.t() + ts @ bw.double().t() + bias.double()
    S = xd.abs() @ wd.abs().t() + ts.abs() @ bw.double().abs().t() + bias.double().abs()
    args = (cols_to(xq, ceil_to(K, 128)).cuda(), xs.cuda(), wq.cuda(), ws.cuda(), N, K, t.cuda(), bw.cuda(),
            bias.cuda(), s)
    y = ext().fused_fp8_gemm_kragged(*args)
    assert_within(y, ref, U * ref.abs() + (K + r) * F32 * S, "y")
    assert torch.equal(y, ext().fused_fp8_gemm_kragged(*args))


# (1, 3) and (3, 1): W holds fewer than four bytes; (129, 1): the last tile does
@pytest.mark.parametrize("N,K", [(N, K) for K in (85, 255, 257, 341) for N in (128, 213)]
                         + [(1, 3), (3, 1), (129, 1), (213, 2)])
def test_kragged_dx(N, K):
    """Exact values on the data of test_ragged_dx; the ragged-N kernel on W zero-padded to whole
    256-column blocks; NaN codes (0xFF) around W must not reach the result."""
    M, Np, Kc = 256, ceil_to(N, 128), ceil_to(K, 256)
    g = gen("kragged-dx", N, K)
    gv, wv = ternary((M, N), g), ternary((N, K), g)
    sg = torch.exp2(torch.randint(0, 2, (M,), generator=g).double())
    ref = (gv @ wv) * sg[:, None]
    assert ref.abs().max() <= 256 and torch.equal(ref.to(BF).double(), ref)
    gq, gs, wq = as_codes(cols_to(gv, Np)), (448 * sg).float().cuda(), as_codes(wv)
    poison(M, K)
    dx = ext().fused_fp8_gemm_dx_kragged(gq, gs, wq, N, K)
    bad = ~(d(dx) == ref)
    assert dx.shape == (M, K) and not bad.any(), f"wrong in columns {bad.any(0).nonzero().flatten().tolist()[:16]}"
    assert torch.equal(dx, ext().fused_fp8_gemm_dx_ragged(gq, gs, as_codes(cols_to(wv, Kc)), N, Kc)[:, :K])
    assert torch.equal(dx, ext().fused_fp8_gemm_dx_kragged(gq, gs, behind_ff(wq), N, K))


def test_kragged_module(monkeypatch):
    """ReLoRaLinear(341 -> 256, fp8) at M = 256: y of the new arm within the kernel's bound on the
    operands it was handed; dx with the switch on within test_fp8_backward_switch's bound for the
    fused arm; with the switch off, and with RELORA_AMD_FP8_RAGGED=0, the materialize arm's dx."""
    from relora_amd.relora import ReLoRaLinear
    M, K, N, r, s = 256, 341, 256, 64, 0.25
    g = gen("kragged-module")
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


def fwd_args():   # the entry point's order: K behind N
    a, out = gemm_args(), {}
    for k, v in a.items():
        out[k] = torch.zeros(256, 100, dtype=torch.uint8, device="cuda") if k == "wq" else v
        if k == "N":
            out["K"] = 100
    return out


FWD = {k: v for k, v in BAD_FWD.items() if k not in ("K-64", "N-128")}
FWD.update({"K-64": ("xq", lambda v: v[:, :64].contiguous(), "K rounded up to 128"), "K-0": ("K", lambda v: 0, "must be > 0"),
            "K-129": ("K", lambda v: 129, "K rounded up to 128"), "K-99": ("K", lambda v: 99, "w codes must hold"),
            "N-128": ("N", lambda v: 128, "w codes must hold"), "xq-misaligned": ("xq", misaligned, "16-byte aligned")})
DX = {k: v for k, v in BAD_DX.items() if k not in ("K-128", "N-64", "wq-misaligned")}
DX.update({"N-64": ("gq", lambda v: v[:, :64].contiguous(), "N rounded up to 128"), "N-0": ("N", lambda v: 0, "must be > 0"),
           "N-129": ("N", lambda v: 129, "N rounded up to 128"), "K-128": ("K", lambda v: 128, "w codes must hold")})
QP = {"x-cpu": ("x", lambda v: v.cpu(), "x must be a GPU tensor"), "x-1d": ("x", lambda v: v.view(-1), "x must be 2-D"),
      "x-strided": ("x", strided, "x must be contiguous"), "x-dtype": ("x", lambda v: v.float(), "x must be bf16"),
      "x-empty": ("x", lambda v: v[:0], "must be > 0")}
ENTRY = {"fused_fp8_gemm_kragged": (FWD, fwd_args),
         "fused_fp8_gemm_dx_kragged": (DX, lambda: dict(dx_args(), wq=torch.zeros(128, 100, dtype=torch.uint8, device="cuda"),
                                                        N=128, K=100)),
         "quantize_rows_fp8_padded": (QP, lambda: dict(x=torch.zeros(4, 33, dtype=BF, device="cuda")))}


@pytest.mark.parametrize("fn,case", [(fn, c) for fn, (bad, _) in ENTRY.items() for c in sorted(bad)])
def test_kragged_rejects(fn, case):
    (key, change, msg), a = ENTRY[fn][0][case], ENTRY[fn][1]()
    a[key] = change(a[key])
    if "dx" in fn:
        a = dict(gq=a["gq"], gs=a["gs"], wq=a["wq"], N=a["N"], K=a["K"])   # the entry point's order
    with pytest.raises(RuntimeError, match=msg):
        getattr(ext(), fn)(*a.values())
