"""Float64 references, error bounds and input builders for norms.hip (RMSNorm,
add+RMSNorm, LayerNorm) and swiglu.hip (SwiGLU, GELU), shared by
tests/test_gpu_norms.py, tests/test_gpu_activations.py and the CPU-only
tests/test_norm_inputs.py.

The references are the mathematical functions in float64, evaluated on the
exact values of the bf16 / fp32 inputs, with the gradients from the closed
formulas of the kernel comments (test_norm_inputs.py pins them against
float64 autograd).

Bounds.  Nothing here comes from running a kernel.  The units:

  U8  = 2^-8    largest relative error of one rounding to bf16
  U23 = 2^-23   per-term unit of an fp32 reduction: a sum of n terms, however
                it is ordered, is within n * 2^-24 * sum|terms| of the exact
                sum, and the rounding of each term (a product) adds 2^-24 of
                it; n * U23 * sum|terms| covers both (n = H for the row sums,
                n = M for the column sums, whose two stages add at most
                rows_per_chunk + chunks <= M + 1 <= 2M times)
  RSQRT_REL     allowance for rsqrtf, see below

An output in bf16 gets one U8 * |ref| per rounding on its path; the fp32
instantiation has none (from_f32<float> is the identity).  Where an output is
a difference of larger terms the fp32 part is written in the magnitudes of
those terms, never in |ref|.

RMSNorm, per row (ss = sum x^2, m = ss / H, ir = rsqrt(m + eps)):
  ss           H * U23 relative (all terms >= 0)
  m + eps      3 more roundings (the division, float(eps), the sum): 3 * U24
  ir           half of that, rsqrt halves a relative error, plus RSQRT_REL:
               E_ir = 0.5 * (H + 2) * U23 + RSQRT_REL            [invrms bound]
  y            h = T(x * ir), y = T(h * w): two roundings to T, two fp32
               products:  ((1 + U8)^2 - 1 + E_ir + U23) * |y|
  dx           dot = mean(g * xh) is an H-term sum of products of four
               factors, one of them ir; xh and the outer factor carry ir too:
               U8 * |dx| + ((H + 4) * U23 + 3 * E_ir) * ir * (|g| + |xh| * mean|g xh|)
               (+ dsum: one more fp32 add, U23 * |dx|, same single rounding)
  dw           M-term column sum of dy * x * ir:
               ((M + 2) * U23 + E_ir) * sum_r |dy x ir|

LayerNorm, per row.  The kernel takes mu0 = fl(sum x) / H, then sums
d = x - mu0 and d^2, and returns mu = mu0 + mean(d), var = mean(d^2) - mean(d)^2
(exact for any shift mu0).  With dl = (H + 1) * U23 * mean|x| >= |mu0 - mu|:
  mean         the H-term sum of d, |d| <= |x - mu| + dl, and two roundings:
               E_mu = U23 * |mu| + (H + 1) * U23 * (mean|x - mu| + dl)  [absolute]
  var          mean(d^2) is an H-term sum of squares of rounded d:
               (H + 2) * U23 * (var + dl^2); mean(d)^2 has value <= dl^2 and
               error 2 * dl * H * U23 * sqrt(var + dl^2) <= H * U23 * (var + 2 dl^2):
               E_var = (3 * H + 8) * U23 * (var + dl^2)                 [absolute]
  invstd       p = (E_var + 4 * U24 * (var + eps)) / (var + eps), the 4 for the
               division, the subtraction, float(eps) and the sum, must be
               < 1/2 for the case to mean anything (ln_reference asserts it);
               E_is = (1 - p)^-1/2 - 1 + RSQRT_REL                      [relative]
               A one-pass var = E[x^2] - mu^2 has (H + 2) * U23 * mean(x^2) in
               place of E_var, which at |mu| >> std is larger than var itself.
  xh           (x - mu) * invstd: shift error a = invstd * E_mu, relative
               error r = E_is + U23
  y            T(xh * w + b), one rounding:
               U8 * |y| + |w| * (a + r * |xh|) + U23 * (|xh w| + |b|)
  dx           invstd * (g - mean g - xh * mean(g xh)), with G = |g| + mean|g|
               + |xh| * mean|g xh|:
               U8 * |dx| + invstd * (((H + 4) * U23 + E_is + 2 r) * G
                                     + a * (|xh| * mean|g| + mean|g xh|))
  dw           (M + 2) * U23 * sum_r |dy xh| + sum_r |dy| * (a + r |xh|)
  db           M * U23 * sum_r |dy|

rsqrtf.  The ROCm documentation installed with the toolchain states no error
bound for rsqrtf, so it is measured on the CPU: torch.rsqrt in fp32 against
float64 over the arguments the tests use (measure_rsqrt below; the CPU test
runs it) is within 1.49 * 2^-24, recorded as RSQRT_MEASURED = 1.5; the
hardware approximation is allowed 4 times that, RSQRT_REL = 6 * 2^-24.

Activations.  Each bf16 output is rounded once: U8 * |ref|, plus an absolute
term for the fp32 formula, a multiple of the natural unit of the output
(|g u|, |dy u|, |dy g|, |x|, |dy|, times 2^-24).  The multiple is 4 times
the largest error of the SAME fp32 formulas evaluated by torch on the CPU
against float64 over the same sweep (measure_activation_units; the CPU test
checks the recorded values), the factor 4 standing for __expf and erff:
see ACT_MEASURED (2.5, 16.3, 2.3, 1.6, 1.9 in that order) and ACT_UNITS.
Results smaller than the smallest normal number, 2^-126 in both types, are
subnormal and may be flushed: TINY is added to every bound.
"""

import math

import torch

U8, U23, U24 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -24

# largest |rsqrt_fp32(a) - a^-1/2| / a^-1/2 seen on the CPU over the tests'
# arguments, in units of 2^-24 (test_norm_inputs.py re-measures and compares)
RSQRT_MEASURED = 1.5
RSQRT_REL = 4 * RSQRT_MEASURED * U24

BF16_MAX = float(torch.finfo(torch.bfloat16).max)
TINY = 2.0 ** -126


def _unit(dtype):
    return U8 if dtype == torch.bfloat16 else 0.0


def worst_fraction(got, ref, bound):
    """max of |got - ref| / bound; an error where the bound is 0 counts as
    inf, a non-finite value as inf"""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    frac = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    frac = torch.where(torch.isfinite(got), frac, torch.full_like(frac, math.inf))
    return frac.max().item() if frac.numel() else 0.0


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------

def rms_reference(x, w, dy, eps, dsum=None):
    """x, dy (and dsum): [M, H]; w: [H]; all in the kernel's dtype T, on the
    CPU.  Returns float64 outputs and bounds."""
    u8 = _unit(x.dtype)
    M, H = x.shape
    x, w, dy = x.double(), w.double(), dy.double()
    ir = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = x * ir
    y = w * xh
    g = dy * w
    dot = (g * xh).mean(-1, keepdim=True)
    dx = ir * (g - xh * dot)
    dx_mag = ir * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if dsum is not None:
        dx = dx + dsum.double()
    dw = (dy * xh).sum(0)
    dw_mag = (dy * xh).abs().sum(0)
    e_ir = 0.5 * (H + 2) * U23 + RSQRT_REL
    return dict(
        y=y, invrms=ir.squeeze(-1), dx=dx, dw=dw,
        invrms_bound=e_ir * ir.squeeze(-1),
        y_bound=((1 + u8) ** 2 - 1 + e_ir + U23) * y.abs(),
        dx_bound=(u8 + U23) * dx.abs() + ((H + 4) * U23 + 3 * e_ir) * dx_mag,
        dw_bound=((M + 2) * U23 + e_ir) * dw_mag,
    )


def ln_reference(x, w, b, dy, eps):
    """LayerNorm with biased variance; arguments as in rms_reference."""
    u8 = _unit(x.dtype)
    M, H = x.shape
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    istd = (var + eps).rsqrt()
    xh = (x - mu) * istd
    y = xh * w + b
    g = dy * w
    mg = g.mean(-1, keepdim=True)
    mgx = (g * xh).mean(-1, keepdim=True)
    dx = istd * (g - mg - xh * mgx)
    a_mg = g.abs().mean(-1, keepdim=True)
    a_mgx = (g * xh).abs().mean(-1, keepdim=True)
    G = g.abs() + a_mg + xh.abs() * a_mgx
    dw = (dy * xh).sum(0)
    db = dy.sum(0)
    # the error model of the two-pass kernel (module docstring)
    dl = (H + 1) * U23 * x.abs().mean(-1, keepdim=True)
    e_mu = U23 * mu.abs() + (H + 1) * U23 * ((x - mu).abs().mean(-1, keepdim=True) + dl)
    e_var = (3 * H + 8) * U23 * (var + dl * dl)
    p = e_var / (var + eps) + 4 * U24
    assert (p < 0.5).all(), "case outside the error model: var + eps too small for |mean|"
    e_is = (1 - p) ** -0.5 - 1 + RSQRT_REL
    a = istd * e_mu
    r = e_is + U23
    return dict(
        y=y, mean=mu.squeeze(-1), invstd=istd.squeeze(-1), dx=dx, dw=dw, db=db,
        mean_bound=e_mu.squeeze(-1),
        invstd_bound=(e_is * istd).squeeze(-1),
        y_bound=u8 * y.abs() + w.abs() * (a + r * xh.abs()) + U23 * ((xh * w).abs() + b.abs()),
        dx_bound=u8 * dx.abs() + istd * (((H + 4) * U23 + e_is + 2 * r) * G
                                         + a * (xh.abs() * a_mg + a_mgx)),
        dw_bound=(M + 2) * U23 * (dy * xh).abs().sum(0)
        + (dy.abs() * (a + r * xh.abs())).sum(0),
        db_bound=M * U23 * dy.abs().sum(0),
    )


def one_pass_invstd_fp32(x, eps):
    """fp32 emulation of var = E[x^2] - mu^2 from one-pass sums (what
    layernorm_fwd_kernel did before the two-pass sum), torch's own summation
    order"""
    f = x.float()
    H = f.shape[-1]
    mu = f.sum(-1) / H
    var = ((f * f).sum(-1) / H - mu * mu).clamp_min(0)
    return torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def two_pass_stats_fp32(x, eps):
    """fp32 emulation of the kernel's two passes, torch's summation order"""
    f = x.float()
    H = f.shape[-1]
    mu0 = f.sum(-1, keepdim=True) / H
    d = f - mu0
    md = d.sum(-1) / H
    var = ((d * d).sum(-1) / H - md * md).clamp_min(0)
    return mu0.squeeze(-1) + md, torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def measure_rsqrt(args):
    """largest relative error of fp32 torch.rsqrt on the CPU, in units of 2^-24"""
    a = args.float().flatten()
    a = a[a > 0]
    ref = a.double().rsqrt()
    return (((torch.rsqrt(a).double() - ref).abs() / ref).max() / U24).item()


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def make_rows(M, H, dtype, seed, scale=None):
    """Ordinary rows: randn times a per-row power of two in 2^-3..2^3 (or
    `scale`), w = 1 + 0.5 randn, b = 0.5 randn, dy = randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g)
    if scale is None:
        x = x * 2.0 ** torch.randint(-3, 4, (M, 1), generator=g).float()
    else:
        x = x * scale
    w = 1 + 0.5 * torch.randn(H, generator=g)
    b = 0.5 * torch.randn(H, generator=g)
    dy = torch.randn(M, H, generator=g)
    return x.to(dtype), w.to(dtype), b.to(dtype), dy.to(dtype)


SPECIAL_ROWS = {
    torch.float32: ("offset100", "offset1000", "constant", "zeros"),
    torch.bfloat16: ("offset256_steps", "offset64", "constant", "zeros"),
}


def special_rows(H, dtype, seed=0):
    """The cancellation rows, one of each kind, in the order of SPECIAL_ROWS:
    fp32  100 + 0.1 randn, 1000 + 0.01 randn, constant 1000.1, zeros
    bf16  256 + {0, 2}, 64 + 0.5 randn, constant 100.5, zeros"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        rows = [100 + 0.1 * torch.randn(H, generator=g),
                1000 + 0.01 * torch.randn(H, generator=g),
                torch.full((H,), 1000.1),
                torch.zeros(H)]
    else:
        rows = [256 + 2.0 * torch.randint(0, 2, (H,), generator=g).float(),
                64 + 0.5 * torch.randn(H, generator=g),
                torch.full((H,), 100.5),
                torch.zeros(H)]
    return torch.stack(rows).to(dtype)


def coverage_case(M, H, dtype, layernorm):
    """Integer data for the row coverage of the column sums, eps = 0.  Row r is
    sigma_r * s with s a fixed +-1 pattern (half +1, half -1 for LayerNorm:
    mean 0, variance 1) and sigma_r = +-1, so mean(x^2) = 1 and xhat = x;
    dy[r, c] = sigma_r * (1 + (r + c) % 3).  Then dy * xhat = s_c * (1 + (r + c) % 3):
    every row moves every dw[c] by 1, 2 or 3 in one direction, and all partial
    sums are integers below 2^24, exact in fp32."""
    g = torch.Generator().manual_seed(M * 131 + H)
    if layernorm:
        assert H % 2 == 0
        s = torch.cat((torch.ones(H // 2), -torch.ones(H - H // 2)))[torch.randperm(H, generator=g)]
    else:
        s = torch.randint(0, 2, (H,), generator=g).float() * 2 - 1
    sigma = torch.randint(0, 2, (M, 1), generator=g).float() * 2 - 1
    r = torch.arange(M)[:, None]
    c = torch.arange(H)[None, :]
    x = sigma * s
    dy = sigma * (1 + (r + c) % 3).float()
    return x.to(dtype), dy.to(dtype)


def coverage_reference(x, dy):
    """exact dw (xhat = x) and db in float64"""
    return (dy.double() * x.double()).sum(0), dy.double().sum(0)


# ---------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------

def bf16_sweep():
    """every bf16 bit pattern that is zero or a finite normal number: 65026 of
    65536, leaving out the 256 inf/NaN patterns and the 254 subnormals"""
    bits = torch.arange(65536, dtype=torch.int32)
    exp = (bits >> 7) & 0xFF
    frac = bits & 0x7F
    keep = (exp != 0xFF) & ((exp != 0) | (frac == 0))
    v = bits[keep].to(torch.int16).view(torch.bfloat16)
    assert v.numel() == 65536 - 510
    return v


SWEEP_U = (1.0, -3.0, 2.0 ** -20, 2.0 ** 20)
SWEEP_DY = (1.0, -0.5)


def fp32_grid():
    pts = torch.tensor([88.0, -88.0, 100.0, -100.0, 1e4, -1e4])
    return torch.cat((torch.linspace(-20, 20, 4096), pts)).float()


def act_reference(g, u, dy):
    """float64 SwiGLU (y, dg, du) and exact-erf GELU of g (y, dx), with the
    natural unit of each output"""
    g, u, dy = g.double(), u.double(), dy.double()
    sig = torch.sigmoid(g)
    # 1 - sigmoid(g) without cancellation
    one_m = torch.sigmoid(-g)
    cdf = 0.5 * torch.erfc(-g / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    ref = {
        "swiglu_y": g * sig * u,
        "swiglu_dg": dy * u * sig * (1 + g * one_m),
        "swiglu_du": dy * g * sig,
        "gelu_y": g * cdf,
        "gelu_dx": dy * (cdf + g * pdf),
    }
    unit = {
        "swiglu_y": (g * u).abs(),
        "swiglu_dg": (dy * u).abs(),
        "swiglu_du": (dy * g).abs(),
        "gelu_y": g.abs(),
        "gelu_dx": dy.abs(),
    }
    return ref, unit


def act_fp32_formulas(g, u, dy):
    """the kernels' fp32 formulas, term for term, by torch on the CPU"""
    g, u, dy = g.float(), u.float(), dy.float()
    sig = 1.0 / (1.0 + torch.exp(-g))
    erf = torch.erf(g * 0.70710678118654752)
    cdf = 0.5 * (1.0 + erf)
    pdf = 0.3989422804014327 * torch.exp(-0.5 * g * g)
    return {
        "swiglu_y": g / (1.0 + torch.exp(-g)) * u,
        "swiglu_dg": dy * u * sig * (1.0 + g * (1.0 - sig)),
        "swiglu_du": dy * (g * sig),
        "gelu_y": 0.5 * g * (1.0 + erf),
        "gelu_dx": dy * (cdf + g * pdf),
    }


def measure_activation_units(g, u, dy):
    """largest |fp32 formula - float64| per output beyond TINY (the underflow
    allowance every bound has), in its unit * 2^-24, over the elements whose
    reference does not overflow"""
    ref, unit = act_reference(g, u, dy)
    got = act_fp32_formulas(g, u, dy)
    out = {}
    for k in ref:
        ok = (ref[k].abs() < BF16_MAX) & (unit[k] > 0)
        err = ((got[k].double() - ref[k]).abs()[ok] - TINY).clamp_min(0)
        out[k] = (err / (unit[k][ok] * U24)).max().item()
    return out


# measured on the CPU by measure_activation_units over the bf16 sweep with every
# (u, dy) pair and over the fp32 grid (test_norm_inputs.py re-measures); the
# kernels are allowed 4 times these for __expf and erff
ACT_MEASURED = {"swiglu_y": 2.5, "swiglu_dg": 16.3, "swiglu_du": 2.3,
                "gelu_y": 1.6, "gelu_dx": 1.9}
ACT_UNITS = {k: 4 * v for k, v in ACT_MEASURED.items()}


def act_bounds(ref, unit, dtype):
    u8 = _unit(dtype)
    return {k: (u8 + U23) * ref[k].abs() + ACT_UNITS[k] * U24 * unit[k] + TINY for k in ref}
