"""The five entry points of fused_gemm.hip (`fused_lora_gemm`, `fused_nf4_gemm`,
`fused_int8_gemm`, and the research variants `fused_lora_gemm3` / `4`) against
float64 CPU references built from the very bf16 tensors handed to the kernel.

* Exact-value grid: inputs whose products and partial sums are all small
  integers, so fp32 accumulation is exact in any order and the bf16 result is
  exact.  `torch.equal`, no tolerance: any wrong index, tile, chunk, absmax
  block or scale fails it.
* Random values with an elementwise a-priori bound (nothing in it is
  measured).  With u = 2^-8 the unit roundoff of bf16 (one round-to-nearest
  is off by at most u*|v|) and n*2^-23*sum|a_i*b_i| the textbook bound of an
  fp32 dot product of length n in any order (twice the round-to-nearest
  constant, which leaves room for a truncating accumulator), a kernel that
  accumulates K + r bf16 products in fp32 and rounds once satisfies
      |got - ref| <= u*|ref| + (K + r)*2^-23*S,
      S = |x|.|W|^T + |t_s|.|bw|^T + |bias|.
  Every bf16 intermediate on a longer path adds u*|that intermediate|,
  propagated through what multiplies it; the module-level tests spell their
  terms out next to the assert.
* Rejected inputs: one case per host check.  They launch nothing: every
  TORCH_CHECK they rely on stands before the entry point's launch.
"""

import itertools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd.ops import functional as Fn
from relora_amd.ops import hip
from relora_amd.ops.functional import _FusedLoRALinear

BF = torch.bfloat16
U = 2.0 ** -8          # bf16 unit roundoff
F32 = 2.0 ** -23       # per-term constant of the fp32 dot-product bound


def ext():
    return hip.ext_or_raise()


def case_gen(*key):
    """Every case draws fresh data from its own seed."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def poison(M, N):
    """Heuristic against stale memory passing for a written tile: fill a
    block of the output's size with NaN and free it, so that the caching
    allocator most likely hands that block to the kernel's `torch::empty`.
    Nothing guarantees the reuse; fresh data per case is the other guard."""
    p = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    del p


def d(t):
    return t.detach().cpu().double()


# ---------------------------------------------------------------------------
# a. exact-value grid
# ---------------------------------------------------------------------------

def ternary(shape, g, density=0.25):
    """{-1, 0, 1}, P(-1) = P(+1) = density / 2."""
    u = torch.rand(shape, generator=g)
    return (u < density / 2).double() - (u > 1 - density / 2).double()


def exact_operands(M, N, K, r, with_bias, g):
    """x, t, bw, bias on the CPU in bf16; lora_scale is 0.5 and t is ternary
    times 2, so the host's t * scale is exact."""
    x = ternary((M, K), g).to(BF)
    t = (2 * ternary((M, r), g)).to(BF) if r else None
    bw = ternary((N, r), g).to(BF) if r else None
    bias = torch.randint(-8, 9, (N,), generator=g).to(BF) if with_bias else None
    return x, t, bw, bias


def nf4_exact_weight(N, K, g):
    """Ternary W with one +-1 forced into every 64-element block: absmax is 1
    and the NF4 codes -1 / 0 / 1 are exact."""
    w = ternary((N * K // 64, 64), g)
    pos = torch.randint(0, 64, (w.shape[0], 1), generator=g)
    sign = torch.randint(0, 2, (w.shape[0], 1), generator=g).double() * 2 - 1
    w.scatter_(1, pos, sign)
    return w.view(N, K).to(BF)


def int8_exact_weight(N, K, g):
    """Integer W whose int8 round trip is exact, with absmax differing from
    block to block so that a wrong absmax index shows.

    A 256-element block holds c * v, v sparse integers in [-3, 3] and c in
    {1, 2} drawn per block, with c * 127 forced into one element: absmax is
    127 * c, the scale absmax / 127 is exactly c and the codes are v and 127.
    The forced element of K-block b sits in column `cols[b]` for every row,
    and the caller zeroes x there: |y| stays under 256 and the bf16 result
    exact (a live +-127 * c per K-block would not)."""
    nb = K // 256
    keep = torch.rand((N, nb, 256), generator=g) < 0.25
    v = torch.randint(1, 4, (N, nb, 256), generator=g).double()
    v = v * (torch.randint(0, 2, (N, nb, 256), generator=g).double() * 2 - 1) * keep
    c = torch.randint(1, 3, (N, nb, 1), generator=g).double()
    w = v * c
    cols = torch.randint(0, 256, (nb,), generator=g)
    for b in range(nb):
        w[:, b, cols[b]] = 127 * c[:, b, 0]
    return w.view(N, K).to(BF), [b * 256 + int(cols[b]) for b in range(nb)]


def assert_exact(got, ref, tile_n, what):
    """`ref` float64.  On a mismatch the message counts the wrong elements per
    256 x tile_n output tile [bm][bn] and names the first one, so that a
    remap, wave or chunk error is readable from the failure."""
    assert ref.abs().max().item() <= 256, "the recipe lost exactness"
    ref_bf = ref.to(BF)
    assert torch.equal(ref_bf.double(), ref), "the recipe lost exactness"
    g = got.cpu()
    bad = ~(g.double() == ref)  # a NaN left in the output counts as wrong
    if bad.any():
        M, N = ref.shape
        tiles = bad.view(M // 256, 256, N // tile_n, tile_n).sum(dim=(1, 3))
        i, j = bad.nonzero()[0].tolist()
        pytest.fail(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; per "
            f"256x{tile_n} tile [bm][bn]: {tiles.tolist()}; first at "
            f"({i}, {j}): got {g[i, j].item()}, want {ref[i, j].item()}")
    assert torch.equal(g, ref_bf)


def run_exact(kernel, M, N, K, r, with_bias):
    g = case_gen(kernel, M, N, K, r, with_bias)
    x, t, bw, bias = exact_operands(M, N, K, r, with_bias, g)
    e = ext()
    if kernel == "nf4":
        w = nf4_exact_weight(N, K, g)
        q, am = e.quantize_nf4(w.cuda().reshape(-1))
        w_ref = e.dequantize_nf4(q, am, N * K, BF).view(N, K).cpu()
        assert am.numel() == N * K // 64 and torch.equal(w_ref, w)
    elif kernel == "int8":
        w, forced = int8_exact_weight(N, K, g)
        x[:, forced] = 0
        q, am = e.quantize_int8(w.cuda().reshape(-1))
        w_ref = e.dequantize_int8(q, am, N * K, BF).view(N, K).cpu()
        assert am.numel() == N * K // 256 and torch.equal(w_ref, w)
        assert sorted(am.unique().tolist()) == [127.0, 254.0]
    else:
        w_ref = ternary((N, K), g).to(BF)

    scale = 0.5
    ref = d(x) @ d(w_ref).t()
    if r:
        ref = ref + (scale * d(t)) @ d(bw).t()
    if with_bias:
        ref = ref + d(bias)

    xg = x.cuda()
    empty = xg.new_empty(0)
    tg = t.cuda() if r else empty
    bg = bw.cuda() if r else empty
    biasg = bias.cuda() if with_bias else empty
    torch.cuda.synchronize()
    poison(M, N)
    if kernel == "nf4":
        got = e.fused_nf4_gemm(xg, q, am, N, tg, bg, biasg, scale)
    elif kernel == "int8":
        got = e.fused_int8_gemm(xg, q, am, N, tg, bg, biasg, scale)
    else:
        fn = {"dense": e.fused_lora_gemm, "gemm3": e.fused_lora_gemm3,
              "gemm4": e.fused_lora_gemm4}[kernel]
        got = fn(xg, w_ref.cuda(), tg, bg, biasg, scale)
    assert got.shape == (M, N) and got.dtype == BF
    assert_exact(got, ref, 128 if kernel == "gemm3" else 256,
                 f"{kernel} M={M} N={N} K={K} r={r} bias={with_bias}")


# nwg = 1, 2, 9 (r8 = 1), 12 (r8 = 4), 8 (r8 = 0), 15 (r8 = 7, q8 = 1),
# 27 (q8 = 3, r8 = 3); KT = 1, 2, 3, 5, 4; RC = 0..4; nbn = 1..4
GRID_SHAPES = [(256, 256, 64, 0), (256, 512, 128, 64), (768, 768, 192, 128),
               (768, 1024, 320, 192), (512, 1024, 256, 256), (1280, 768, 64, 64),
               (2304, 768, 128, 128)]
# the same grids and ranks with 1, 2, 3 absmax blocks per row (KT = 4, 8, 12)
INT8_SHAPES = [(M, N, k, r) for (M, N, _, r), k in
               zip(GRID_SHAPES, (256, 512, 768, 256, 512, 768, 256))]
# every branch of the vmcnt ladder (ST = 1..5), odd and even 32-chunk counts,
# on the 9- and the 12-block grid
GEMM4_SHAPES = [(M, N, K, r) for (M, N), K, r in itertools.product(
    [(768, 768), (768, 1024)], (32, 64, 96, 128, 160), (0, 32, 96, 256))]
# fused_lora_gemm3 maps blocks to 256 x 128 tiles (nbn = N / 128) after the
# same remap: 9 blocks (N = 384 is no multiple of 256) over K x r, then 12, 10,
# 15 and 25 blocks (r8 = 4, 2, 7, 1; q8 up to 3)
GEMM3_SHAPES = ([(768, 384, K, r) for K in (64, 128, 192, 320) for r in (0, 64, 128)]
                + [(768, 512, 128, 64), (512, 640, 192, 128), (1280, 384, 64, 0),
                   (1280, 640, 320, 128)])

EXACT_CASES = ([("dense",) + s for s in GRID_SHAPES]
               + [("nf4",) + s for s in GRID_SHAPES]
               + [("int8",) + s for s in INT8_SHAPES]
               + [("gemm4",) + s for s in GEMM4_SHAPES]
               + [("gemm3",) + s for s in GEMM3_SHAPES])


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("kernel,M,N,K,r", EXACT_CASES,
                         ids=["{}-{}x{}x{}-r{}".format(*c) for c in EXACT_CASES])
def test_exact_value_grid(kernel, M, N, K, r, with_bias):
    run_exact(kernel, M, N, K, r, with_bias)


@pytest.mark.parametrize("mode,N,K", [("nf4", 768, 512), ("int8", 768, 768)])
def test_quantized_kernels_stage_the_materialized_weight(mode, N, K):
    """x = identity: y^T is the B image the kernel staged, element for
    element (the other K - 1 products of every sum are zeros).  It must be
    bit-equal to what dequantize_* returns, which is what the backward and the
    references use as W."""
    g = case_gen("identity", mode, N, K)
    w = (torch.randn(N, K, generator=g) * 0.1).to(BF).cuda()
    e = ext()
    if mode == "nf4":
        q, am = e.quantize_nf4(w.reshape(-1))
        wd = e.dequantize_nf4(q, am, N * K, BF).view(N, K)
        fn = e.fused_nf4_gemm
    else:
        q, am = e.quantize_int8(w.reshape(-1))
        wd = e.dequantize_int8(q, am, N * K, BF).view(N, K)
        fn = e.fused_int8_gemm
    x = torch.eye(K, dtype=BF, device="cuda")
    empty = x.new_empty(0)
    poison(K, N)
    y = fn(x, q, am, N, empty, empty, empty, 1.0)
    assert torch.equal(y.t().contiguous(), wd), \
        f"{int((y.t() != wd).sum())} staged elements differ"


# ---------------------------------------------------------------------------
# b. random values, derived elementwise bound
# ---------------------------------------------------------------------------

def assert_within(got, ref, bound, what):
    err = (d(got) - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        ratio = err / bound.clamp_min(1e-300)
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        pytest.fail(f"{what}: {int((~ok).sum())} of {ok.numel()} elements past "
                    f"the bound; worst at {idx}: err {err[idx].item():.3e}, "
                    f"bound {bound[idx].item():.3e}, ref {ref[idx].item():.3e}")
    return (err / bound.clamp_min(1e-300)).max().item()


RANDOM_CASES = [("dense", 768, 768, 192, 128), ("dense", 768, 1024, 320, 192),
                ("nf4", 768, 768, 192, 128), ("nf4", 768, 1024, 320, 192),
                # fused_int8_gemm needs K % 256 == 0: the nearest K it accepts
                ("int8", 768, 768, 256, 128), ("int8", 768, 1024, 512, 192)]


@pytest.mark.parametrize("scale", [0.25, 1.0], ids=["s0.25", "s1-nocopy"])
@pytest.mark.parametrize("kernel,M,N,K,r", RANDOM_CASES,
                         ids=["{}-{}x{}x{}-r{}".format(*c) for c in RANDOM_CASES])
def test_random_values_within_derived_bound(kernel, M, N, K, r, scale):
    """|got - ref| <= 2^-8 |ref| + (K + r) 2^-23 S elementwise, with
    S = |x|.|W|^T + |t_s|.|bw|^T + |bias| in float64 (module docstring).

    The first term is the one round-to-nearest to bf16 of the result, the
    second the fp32 dot product of length K + r in any order.  The reference
    uses t_s = bf16(t * scale), which is what the host hands the kernel (for
    scale == 1.0, t itself without a copy), and for the quantized kernels
    the dequantized bf16 W, which the kernels stage bit for bit
    (test_quantized_kernels_stage_the_materialized_weight).  Two calls on the
    same inputs are bit-equal."""
    g = case_gen("random", kernel, M, N, K, r, scale)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(BF)  # noqa: E731
    x, w, t, bw, bias = rnd(M, K), rnd(N, K), rnd(M, r), rnd(N, r), rnd(N)
    e = ext()
    xg, tg, bg, biasg = x.cuda(), t.cuda(), bw.cuda(), bias.cuda()
    if kernel == "nf4":
        q, am = e.quantize_nf4(w.cuda().reshape(-1))
        w = e.dequantize_nf4(q, am, N * K, BF).view(N, K).cpu()
        call = lambda: e.fused_nf4_gemm(xg, q, am, N, tg, bg, biasg, scale)  # noqa: E731
    elif kernel == "int8":
        q, am = e.quantize_int8(w.cuda().reshape(-1))
        w = e.dequantize_int8(q, am, N * K, BF).view(N, K).cpu()
        call = lambda: e.fused_int8_gemm(xg, q, am, N, tg, bg, biasg, scale)  # noqa: E731
    else:
        wg = w.cuda()
        call = lambda: e.fused_lora_gemm(xg, wg, tg, bg, biasg, scale)  # noqa: E731

    t_s = (t.float() * scale).to(BF)
    ref = d(x) @ d(w).t() + d(t_s) @ d(bw).t() + d(bias)
    S = d(x).abs() @ d(w).abs().t() + d(t_s).abs() @ d(bw).abs().t() + d(bias).abs()
    bound = U * ref.abs() + (K + r) * F32 * S

    poison(M, N)
    got = call()
    worst = assert_within(got, ref, bound, f"{kernel} {M}x{N}x{K} r={r} s={scale}")
    print(f"{kernel} {M}x{N}x{K} r={r} s={scale}: worst err/bound {worst:.3f}")
    poison(M, N)
    assert torch.equal(call(), got)


# ---------------------------------------------------------------------------
# c. module level
# ---------------------------------------------------------------------------

def lora_linear_reference(x, W, bias, A, B, s):
    """float64 y = x W^T + bias + (s x A^T) B^T from the bf16 operands, and
    the pieces the bounds are made of."""
    x, W, A, B = d(x), d(W), d(A), d(B)
    b = d(bias) if bias is not None else torch.zeros(W.shape[0], dtype=torch.float64)
    t = x @ A.t()
    main = x @ W.t() + b
    lora = (s * t) @ B.t()
    return dict(x=x, W=W, A=A, B=B, b=b, t=t, main=main, lora=lora, y=main + lora)


@pytest.mark.parametrize("zero_w", [False, True], ids=["W", "W0"])
def test_fused_lora_linear_both_arms_against_float64(zero_w, monkeypatch):
    """_FusedLoRALinear at 9 blocks, K <= 1024 (the fused_lora_gemm arm), and
    the same call with the fused GEMM switched off (library GEMM +
    lora_add_nt_), against one float64 reference.  With W = 0, y is the LoRA
    term alone: a lost chunk or a wrong scale is a 100 % error."""
    M, K, N, r, s = 768, 256, 768, 128, 0.25  # s a power of two: s*t, s*B exact
    g = case_gen("fused_linear", zero_w)
    x = torch.randn(M, K, generator=g).to(BF).cuda()
    W = (torch.zeros(N, K) if zero_w else torch.randn(N, K, generator=g) * 0.05).to(BF).cuda()
    A = (torch.randn(r, K, generator=g) * 0.05).to(BF).cuda()
    B = (torch.randn(N, r, generator=g) * 0.1).to(BF).cuda()
    bias = None if zero_w else (torch.randn(N, generator=g) * 0.1).to(BF).cuda()
    R = lora_linear_reference(x, W, bias, A, B, s)

    # fused arm: t_u = bf16(x A^T) is the one bf16 intermediate (s * t_u is
    # exact).  Its rounding, u*|t|, reaches y through |s B|; the rest is the
    # bound of the kernel for the operands it was handed.
    S = R["x"].abs() @ R["W"].abs().t() + (s * R["t"]).abs() @ R["B"].abs().t() + R["b"].abs()
    fused = (U * R["y"].abs() + (K + r) * F32 * S
             + U * (R["t"].abs() @ (s * R["B"]).abs().t()))
    # composed arm: F.linear rounds x W^T + bias to bf16, lora_add_nt_ rounds
    # its product t_u (sB)^T to bf16 before it adds: two more intermediates.
    composed = fused + U * R["main"].abs() + U * R["lora"].abs()

    assert Fn._use_fused_k1(x, W, A)
    poison(M, N)
    y = _FusedLoRALinear.apply(x, W, bias, A, B, s, 0.0, True)
    assert_within(y, R["y"], fused, "fused arm")

    monkeypatch.setattr(Fn, "_FUSED_K1", "0")
    assert not Fn._use_fused_k1(x, W, A)
    y2 = _FusedLoRALinear.apply(x, W, bias, A, B, s, 0.0, True)
    assert_within(y2, R["y"], composed, "composed arm")


@pytest.mark.parametrize("M", [256, 200], ids=["fused", "materialize"])
@pytest.mark.parametrize("mode", ["4bit", "8bit"])
def test_quantized_relora_linear_fwd_bwd_against_float64(mode, M):
    """ReLoRaLinear(quantize=...) at p = 0: y, dx, dA and dB against float64
    autograd over the materialized weight.  M = 256 runs the dequant-fused
    kernels, M = 200 the materialize + library GEMM + lora_add_nt_ path."""
    from relora_amd.relora import ReLoRaLinear

    K = N = 256
    r, s = 64, 0.25  # alpha / r, a power of two: s*t and s*B are exact in bf16
    g = case_gen("quantized_module", mode, M)
    lin = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.0, quantize=mode,
                       bias=True, weight_data=torch.randn(N, K, generator=g) * 0.05)
    with torch.no_grad():
        lin.lora_A.weight.copy_(torch.randn(r, K, generator=g) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(N, r, generator=g) * 0.1)
        lin.bias.copy_(torch.randn(N, generator=g) * 0.1)
    lin = lin.to(device="cuda", dtype=BF)
    assert lin.training and lin._post_lora_scale() == s
    x = torch.randn(M, K, generator=g).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(M, N, generator=g).to(BF).cuda()

    y = lin(x)
    y.backward(dy)
    A, B = lin.lora_A.weight, lin.lora_B.weight
    Wd = lin.weight.materialize(BF)

    x64, A64, B64 = (d(v).requires_grad_(True) for v in (x, A, B))
    W64, b64, dy64 = d(Wd), d(lin.bias), d(dy)
    y64 = x64 @ W64.t() + b64 + (s * (x64 @ A64.t())) @ B64.t()
    y64.backward(dy64)
    xa, Aa, sBa, Wa, dya = (v.detach().abs() for v in (x64, A64, s * B64, W64, dy64))
    t = (x64 @ A64.t()).detach()      # [M, r], bf16 on the GPU (t_u)
    us = dy64 @ (s * B64).detach()    # [M, r], bf16 on the GPU (u_s)
    xA, dysB = xa @ Aa.t(), dya @ sBa  # what bounds |t|, |us| term by term

    # y.  Every path: t_u rounded (u*|t| through |sB|); fp32 sums of length K
    # for t_u and K + r for y, (2K + r) 2^-24 <= (K + r) 2^-23 of the absolute
    # sums; the result rounded.  The materialize path also rounds
    # x W^T + bias (F.linear) and the product t_u (sB)^T (lora_add_nt_).
    main = (x64 @ W64.t() + b64).detach()
    lora = y64.detach() - main
    by = (U * y64.detach().abs() + U * (t.abs() @ sBa.t())
          + (K + r) * F32 * (xa @ Wa.t() + xA @ sBa.t() + b64.abs()))
    if M % 256:
        by = by + U * main.abs() + U * lora.abs()
    assert_within(y, y64.detach(), by, "y")

    # dx = bf16(bf16(dy W) + bf16(bf16(dy sB) A)): the result and three
    # intermediates (dy W; u_s, reaching dx through |A|; the product u_s A that
    # lora_add_nn_ rounds before it adds), fp32 sums of length N (dy W and
    # u_s) and r.
    bdx = (U * x64.grad.abs() + U * (dy64 @ W64).abs() + U * (us @ A64.detach()).abs()
           + U * (us.abs() @ Aa) + (N + r) * F32 * (dya @ Wa + dysB @ Aa))
    assert_within(x.grad, x64.grad, bdx, "dx")

    # dA = bf16(u_s^T x): the result, u_s rounded (through |x|), fp32 sums of
    # length N (u_s) and M (fp32 partial planes, one rounding at the end).
    bdA = (U * A64.grad.abs() + U * (us.abs().t() @ xa)
           + (M + N) * F32 * (dysB.t() @ xa))
    assert_within(A.grad, A64.grad, bdA, "dA")

    # dB = bf16(s dy^T t_u): the result, t_u rounded (through |dy|), fp32 sums
    # of length K (t_u) and M; s is a power of two.
    bdB = (U * B64.grad.abs() + U * s * (dya.t() @ t.abs())
           + (M + K) * F32 * s * (dya.t() @ xA))
    assert_within(B.grad, B64.grad, bdB, "dB")


# ---------------------------------------------------------------------------
# rejected inputs: every check below fires before the entry point's launch
# ---------------------------------------------------------------------------

ENTRIES = ["fused_lora_gemm", "fused_lora_gemm3", "fused_lora_gemm4",
           "fused_nf4_gemm", "fused_int8_gemm"]
QUANT = ("fused_nf4_gemm", "fused_int8_gemm")


def valid_args(entry):
    """Well-formed arguments (never passed on unchanged), M = N = K = 256,
    r = 64, as a dict in the entry point's order."""
    M = N = K = 256
    r = 64
    z = lambda *s: torch.zeros(*s, dtype=BF, device="cuda")  # noqa: E731
    a = dict(x=z(M, K))
    if entry == "fused_nf4_gemm":
        a.update(qw=torch.zeros(N * K // 2, dtype=torch.uint8, device="cuda"),
                 amax=torch.ones(N * K // 64, device="cuda"), N=N)
    elif entry == "fused_int8_gemm":
        a.update(qw=torch.zeros(N * K, dtype=torch.int8, device="cuda"),
                 amax=torch.ones(N * K // 256, device="cuda"), N=N)
    else:
        a.update(w=z(N, K))
    a.update(t=z(M, r), bw=z(N, r), bias=z(N), scale=0.5)
    return a


def strided(t):
    """Same shape, dtype, device and values; not contiguous."""
    big = torch.zeros(*t.shape[:-1], t.shape[-1] * 2, dtype=t.dtype, device=t.device)
    return big[..., ::2]


COMMON_BAD = {
    "x-fp32": (dict(x=lambda a: a["x"].float()), "x must be bf16"),
    "x-cpu": (dict(x=lambda a: a["x"].cpu()), "x must be a GPU tensor"),
    "x-strided": (dict(x=lambda a: strided(a["x"])), "x must be contiguous"),
    "x-K0": (dict(x=lambda a: a["x"][:, :0].contiguous()), "K must be > 0"),
    "t-half-rows": (dict(t=lambda a: a["t"][:128].contiguous()), r"t must be \[M, r\]"),
    "t-fp32": (dict(t=lambda a: a["t"].float()), "t must be bf16"),
    "t-strided": (dict(t=lambda a: strided(a["t"])), "t must be contiguous"),
    "t-strided-scale1": (dict(t=lambda a: strided(a["t"]), scale=lambda a: 1.0),
                         "t must be contiguous"),
    "t-half-rows-scale1": (dict(t=lambda a: a["t"][:128].contiguous(),
                                scale=lambda a: 1.0), r"t must be \[M, r\]"),
    "t-cpu": (dict(t=lambda a: a["t"].cpu()), "t must be on x's device"),
    "r-320": (dict(t=lambda a: a["t"].new_zeros(256, 320),
                   bw=lambda a: a["bw"].new_zeros(256, 320)), "r must be a multiple"),
    "r-48": (dict(t=lambda a: a["t"].new_zeros(256, 48),
                  bw=lambda a: a["bw"].new_zeros(256, 48)), "r must be a multiple"),
    "bw-half-rows": (dict(bw=lambda a: a["bw"][:128].contiguous()), r"bw must be \[N, r\]"),
    "bw-half-rank": (dict(bw=lambda a: a["bw"][:, :32].contiguous()), r"bw must be \[N, r\]"),
    "bw-fp32": (dict(bw=lambda a: a["bw"].float()), "bw must be bf16"),
    "bw-strided": (dict(bw=lambda a: strided(a["bw"])), "bw must be contiguous"),
    "bw-cpu": (dict(bw=lambda a: a["bw"].cpu()), "bw must be on x's device"),
    "bias-short": (dict(bias=lambda a: a["bias"][:128].contiguous()),
                   "bias must have N elements"),
    "bias-fp32": (dict(bias=lambda a: a["bias"].float()), "bias must be bf16"),
    "bias-strided": (dict(bias=lambda a: strided(a["bias"])), "bias must be contiguous"),
    "bias-cpu": (dict(bias=lambda a: a["bias"].cpu()), "bias must be on x's device"),
}
DENSE_BAD = {
    "w-fp32": (dict(w=lambda a: a["w"].float()), "w must be bf16"),
    "w-cpu": (dict(w=lambda a: a["w"].cpu()), "w must be on x's device"),
    "w-strided": (dict(w=lambda a: strided(a["w"])), "w must be contiguous"),
    "w-K-mismatch": (dict(w=lambda a: a["w"][:, :128].contiguous()), "K mismatch"),
    "N0": (dict(w=lambda a: a["w"][:0].contiguous(), bw=lambda a: a["bw"][:0].contiguous(),
                bias=lambda a: a["bias"][:0].contiguous()), "N must be > 0"),
}
QUANT_BAD = {
    "qw-strided": (dict(qw=lambda a: strided(a["qw"])), "qw must be contiguous"),
    "qw-cpu": (dict(qw=lambda a: a["qw"].cpu()), "qw must be on x's device"),
    "qw-short": (dict(qw=lambda a: a["qw"][:-32].contiguous()), "packed weight size mismatch"),
    "qw-dtype": (dict(qw=lambda a: a["qw"].to(torch.int16)), "qw must be"),
    "amax-short": (dict(amax=lambda a: a["amax"][:-1].contiguous()), "absmax must hold"),
    "amax-half": (dict(amax=lambda a: a["amax"][:a["amax"].numel() // 2].contiguous()),
                  "absmax must hold"),
    "amax-bf16": (dict(amax=lambda a: a["amax"].to(BF)), "absmax must be fp32"),
    "amax-fp64": (dict(amax=lambda a: a["amax"].double()), "absmax must be fp32"),
    "amax-strided": (dict(amax=lambda a: strided(a["amax"])), "absmax must be contiguous"),
    "amax-cpu": (dict(amax=lambda a: a["amax"].cpu()), "absmax must be on x's device"),
    "N0": (dict(N=lambda a: 0, qw=lambda a: a["qw"][:0].contiguous(),
                amax=lambda a: a["amax"][:0].contiguous()), "N must be > 0"),
}
REJECT_CASES = []
for _e in ENTRIES:
    for _table in (COMMON_BAD, QUANT_BAD if _e in QUANT else DENSE_BAD):
        REJECT_CASES += [(_e, _name) for _name in _table]
REJECT_CASES.append(("fused_lora_gemm3", "r-192"))


@pytest.mark.parametrize("entry,name", REJECT_CASES,
                         ids=[f"{e}-{n}" for e, n in REJECT_CASES])
def test_rejected_inputs(entry, name):
    if name == "r-192":  # a rank the other entry points take, gemm3 does not
        change = dict(t=lambda a: a["t"].new_zeros(256, 192),
                      bw=lambda a: a["bw"].new_zeros(256, 192))
        msg = "r must be a multiple"
    else:
        table = COMMON_BAD if name in COMMON_BAD else (
            QUANT_BAD if entry in QUANT else DENSE_BAD)
        change, msg = table[name]
    args = valid_args(entry)
    args.update({k: f(args) for k, f in change.items()})
    with pytest.raises(RuntimeError, match=msg):
        getattr(ext(), entry)(*args.values())
