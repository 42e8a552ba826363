"""norms.hip (RMSNorm, add+RMSNorm, LayerNorm, the two-stage dW/db sums)
against the float64 references of tests/norm_common.py, whose docstring
derives every bound used here: row lengths at every path of the row kernels,
the saved statistics, rows with a common offset, constant and zero rows, eps,
the chunking of the column sums, add+RMSNorm against the unfused kernels bit
for bit, one rejected input per host check, and the dispatch of ops.rmsnorm /
ops.add_rmsnorm / ops.layernorm.

Row lengths: 1 and 7 are shorter than one 8-wide vector; 9, 12, 100, 513,
2049, 5461 have a scalar tail and leave every later row off a 16-byte
boundary; 504 / 512 / 513 / 520 and 2048 / 2049 / 2056 sit on both sides of
the steps of norm_block (64, 256, 512 threads); 520, 2056 and 4104 are one
vector more than one pass of those blocks covers, so the strided second pass
runs."""

import pytest
import torch

import norm_common as nc
from relora_amd import ops
from relora_amd.ops import functional as Fn
from relora_amd.ops import hip

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [BF16, FP32]
H_GRID = [1, 7, 8, 9, 12, 100, 504, 512, 513, 520, 2048, 2049, 2056, 4096, 4104, 5461]


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _fractions(tag, ref, **got):
    """worst error / bound per output; prints them, then asserts all <= 1"""
    worst = {k: nc.worst_fraction(v, ref[k], ref[k + "_bound"]) for k, v in got.items()}
    print(f"NORM_FRAC {tag} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


def _rms(x, w, dy, eps):
    ext = hip.ext()
    xg, wg, dyg = _cuda(x, w, dy)
    y, ir = ext.rmsnorm_fwd(xg, wg, eps)
    assert ir.dtype == FP32 and ir.shape == (x.shape[0],) and y.dtype == x.dtype
    dx, dw = ext.rmsnorm_bwd(xg, wg, ir, dyg)
    assert dw.dtype == FP32 and dw.shape == (x.shape[1],) and dx.dtype == x.dtype
    torch.cuda.synchronize()
    return dict(y=y, invrms=ir, dx=dx, dw=dw)


def _ln(x, w, b, dy, eps):
    ext = hip.ext()
    xg, wg, bg, dyg = _cuda(x, w, b, dy)
    y, mean, invstd = ext.layernorm_fwd(xg, wg, bg, eps)
    assert mean.dtype == FP32 and invstd.dtype == FP32 and mean.shape == (x.shape[0],)
    dx, dw, db = ext.layernorm_bwd(xg, wg, mean, invstd, dyg)
    assert dw.dtype == FP32 and db.dtype == FP32 and dw.shape == db.shape == (x.shape[1],)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, dx=dx, dw=dw, db=db)


# -- 1. row lengths -------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", H_GRID)
def test_rmsnorm_row_lengths(H, dtype):
    x, w, _, dy = nc.make_rows(4, H, dtype, seed=H)
    ref = nc.rms_reference(x, w, dy, 1e-6)
    _fractions(f"rms H{H} {_name(dtype)}", ref, **_rms(x, w, dy, 1e-6))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", H_GRID)
def test_layernorm_row_lengths(H, dtype):
    x, w, b, dy = nc.make_rows(5, H, dtype, seed=1000 + H)
    ref = nc.ln_reference(x, w, b, dy, 1e-5)
    _fractions(f"ln H{H} {_name(dtype)}", ref, **_ln(x, w, b, dy, 1e-5))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", H_GRID)
def test_add_rmsnorm_row_lengths(H, dtype):
    """sum is the exactly rounded x + res; y, invrms, dw (and dx with a zero
    dsum) are bit-equal to the unfused kernels on that sum; dx with a dsum is
    held to the float64 bound with its single rounding"""
    ext = hip.ext()
    eps = 1e-6
    x, w, _, dy = nc.make_rows(3, H, dtype, seed=2000 + H)
    res, _, _, dsum = nc.make_rows(3, H, dtype, seed=3000 + H)
    xg, rg, wg, dyg, dsg = _cuda(x, res, w, dy, dsum)
    y, s, ir = ext.rmsnorm_fwd_add(xg, rg, wg, eps)
    want_s = (x.float() + res.float()).to(dtype)
    assert torch.equal(s.cpu(), want_s)
    y0, ir0 = ext.rmsnorm_fwd(s, wg, eps)
    assert torch.equal(y, y0) and torch.equal(ir, ir0)
    dx0, dw0 = ext.rmsnorm_bwd(s, wg, ir, dyg)
    dxz, dwz = ext.rmsnorm_bwd_add(s, wg, ir, dyg, torch.zeros_like(dyg))
    assert torch.equal(dxz, dx0) and torch.equal(dwz, dw0)
    dx1, dw1 = ext.rmsnorm_bwd_add(s, wg, ir, dyg, dsg)
    assert torch.equal(dw1, dw0)
    ref = nc.rms_reference(want_s, w, dy, eps)
    _fractions(f"add H{H} {_name(dtype)}", ref, y=y, invrms=ir, dx=dx0, dw=dw0)
    ref1 = nc.rms_reference(want_s, w, dy, eps, dsum=dsum)
    _fractions(f"add+dsum H{H} {_name(dtype)}", ref1, dx=dx1)


@pytest.mark.parametrize("H", [12, 520])
@pytest.mark.parametrize("with_dsum", [False, True])
def test_add_rmsnorm_autograd(H, with_dsum):
    """ops.add_rmsnorm in bf16, with and without a gradient into the sum,
    returns what the extension entries give"""
    ext = hip.ext()
    x, w, _, dy = nc.make_rows(3, H, BF16, seed=H)
    res, _, _, dsum = nc.make_rows(3, H, BF16, seed=H + 1)
    xg, rg, wg, dyg, dsg = _cuda(x, res, w, dy, dsum)
    xa, ra, wa = (t.clone().requires_grad_() for t in (xg, rg, wg))
    normed, s = ops.add_rmsnorm(xa, ra, wa, 1e-6)
    if with_dsum:
        gx, gr, gw = torch.autograd.grad((normed, s), (xa, ra, wa), (dyg, dsg))
    else:
        gx, gr, gw = torch.autograd.grad(normed, (xa, ra, wa), dyg)
    y0, s0, ir0 = ext.rmsnorm_fwd_add(xg, rg, wg, 1e-6)
    dx0, dw0 = ext.rmsnorm_bwd_add(s0, wg, ir0, dyg, dsg if with_dsum else torch.zeros_like(dsg))
    assert torch.equal(normed, y0) and torch.equal(s, s0)
    assert torch.equal(gx, dx0) and torch.equal(gr, dx0)
    assert torch.equal(gw, dw0.to(BF16))


# -- 2. offset, constant and zero rows --------------------------------------------

def _mixed_rows(H, dtype):
    """special rows interleaved with ordinary ones, in one launch"""
    sp = nc.special_rows(H, dtype, seed=H)
    x, w, b, dy = nc.make_rows(2 * sp.shape[0], H, dtype, seed=4000 + H)
    x[1::2] = sp
    return x, w, b, dy, list(range(1, x.shape[0], 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [100, 768])
def test_layernorm_offset_constant_zero_rows(H, dtype):
    """|mean| >> std: the rows on which var = E[x^2] - mean^2 cancels
    (tests/test_norm_inputs.py shows the one-pass formula far outside these
    bounds on the same rows)"""
    eps = 1e-5
    x, w, b, dy, where = _mixed_rows(H, dtype)
    ref = nc.ln_reference(x, w, b, dy, eps)
    got = _ln(x, w, b, dy, eps)
    for name, r in zip(nc.SPECIAL_ROWS[dtype], where):
        f = nc.worst_fraction(got["invstd"][r], ref["invstd"][r], ref["invstd_bound"][r])
        rel = abs(got["invstd"][r].item() / ref["invstd"][r].item() - 1)
        print(f"NORM_OFFSET ln H{H} {_name(dtype)} {name}: invstd rel err {rel:.3e} "
              f"= {f:.3f} of bound")
    _fractions(f"ln-special H{H} {_name(dtype)}", ref, **got)
    zero, const = where[3], where[2]
    assert not x[zero].any() and (x[const] == x[const][0]).all()
    # constant and zero rows: var = 0, so invstd = rsqrt(eps) and y = b
    for r in (zero, const):
        assert abs(ref["invstd"][r].item() - eps ** -0.5) < 1e-9 * eps ** -0.5
    assert torch.equal(got["y"][zero].cpu(), b)
    assert got["mean"][zero].item() == 0.0
    # dx = rsqrt(eps) * (g - mean g) on the zero row
    g = dy[zero].double() * w.double()
    assert torch.allclose(ref["dx"][zero], eps ** -0.5 * (g - g.mean()), rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H", [100, 768])
def test_rmsnorm_offset_constant_zero_rows(H, dtype):
    eps = 1e-5
    x, w, _, dy, where = _mixed_rows(H, dtype)
    ref = nc.rms_reference(x, w, dy, eps)
    got = _rms(x, w, dy, eps)
    _fractions(f"rms-special H{H} {_name(dtype)}", ref, **got)
    zero = where[3]
    assert abs(ref["invrms"][zero].item() - eps ** -0.5) < 1e-9 * eps ** -0.5
    assert not got["y"][zero].any()
    g = dy[zero].double() * w.double()
    assert torch.allclose(ref["dx"][zero], eps ** -0.5 * g, rtol=1e-12, atol=0)


# -- 3. eps ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("eps,scale", [(1e-6, None), (1e-5, None), (1e-2, 1e-3)])
def test_eps(eps, scale, dtype):
    """at eps = 1e-2 and x ~ 1e-3 randn eps is 10^4 times the mean square: a
    kernel that dropped it, or added it after the rsqrt, is off by 100x"""
    H = 520
    x, w, b, dy = nc.make_rows(4, H, dtype, seed=77, scale=scale)
    if scale is not None:
        assert (x.double().pow(2).mean(-1) < 1e-3 * eps).all()
    _fractions(f"rms eps{eps} {_name(dtype)}", nc.rms_reference(x, w, dy, eps),
               **_rms(x, w, dy, eps))
    _fractions(f"ln eps{eps} {_name(dtype)}", nc.ln_reference(x, w, b, dy, eps),
               **_ln(x, w, b, dy, eps))
    ext = hip.ext()
    xg, wg, dyg = _cuda(x, w, dy)
    y, s, ir = ext.rmsnorm_fwd_add(xg, torch.zeros_like(xg), wg, eps)
    y0, ir0 = ext.rmsnorm_fwd(xg, wg, eps)
    assert torch.equal(s, xg) and torch.equal(y, y0) and torch.equal(ir, ir0)


# -- 4. the chunked column sums -----------------------------------------------------------

# reduce_chunks: ceil(M / 64) chunks up to 256.  1, 63, 64: one chunk; 65, 129:
# a ragged last chunk; 4097: 65 chunks of 64 rows (the last holds one row);
# 16384: 256 full chunks; 16385 and 16640: 65 rows per chunk, so the last
# chunks start past M and must store 0.  H = 255 / 256 / 257: one column
# block short of, equal to and over the 256 columns of a block.
CHUNK_SHAPES = [(1, 24), (63, 24), (64, 24), (65, 24), (129, 24), (4097, 24),
                (16384, 8), (16385, 8), (16640, 8), (130, 255), (130, 256), (130, 257)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", CHUNK_SHAPES)
def test_column_sums_values(M, H, dtype):
    x, w, b, dy = nc.make_rows(M, H, dtype, seed=M + H)
    r = _rms(x, w, dy, 1e-6)
    _fractions(f"rms-dw M{M} H{H} {_name(dtype)}", nc.rms_reference(x, w, dy, 1e-6),
               dw=r["dw"], invrms=r["invrms"])
    g = _ln(x, w, b, dy, 1e-5)
    _fractions(f"ln-dwdb M{M} H{H} {_name(dtype)}", nc.ln_reference(x, w, b, dy, 1e-5),
               dw=g["dw"], db=g["db"], mean=g["mean"], invstd=g["invstd"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", CHUNK_SHAPES)
def test_rmsnorm_dw_counts_every_row_once(M, H, dtype):
    """integer data (norm_common.coverage_case), eps = 0: dropping or doubling
    one row moves every dw[c] by at least 1; compared at a relative 2^-20.
    rmsnorm_bwd and rmsnorm_bwd_add share the reduction and must agree, and a
    second call gives the same bits (no atomics)."""
    ext = hip.ext()
    x, dy = nc.coverage_case(M, H, dtype, layernorm=False)
    want, _ = nc.coverage_reference(x, dy)
    assert (want.abs() >= M).all()
    xg, dyg = _cuda(x, dy)
    wg = torch.ones(H, dtype=dtype, device="cuda")
    _, ir = ext.rmsnorm_fwd(xg, wg, 0.0)
    dw = ext.rmsnorm_bwd(xg, wg, ir, dyg)[1]
    err = ((dw.double().cpu() - want).abs() / want.abs()).max().item()
    print(f"NORM_ROWS rms M{M} H{H} {_name(dtype)} max rel err {err:.3e}")
    assert err <= 2.0 ** -20
    assert torch.equal(dw, ext.rmsnorm_bwd(xg, wg, ir, dyg)[1])
    assert torch.equal(dw, ext.rmsnorm_bwd_add(xg, wg, ir, dyg, dyg)[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("M,H", [s for s in CHUNK_SHAPES if s[1] % 2 == 0])
def test_layernorm_dwdb_count_every_row_once(M, H, dtype):
    """as above with rows of mean 0 and variance 1 (they need an even H; the
    odd column counts 255 and 257 are in test_column_sums_values); db is a
    plain sum of integers"""
    ext = hip.ext()
    x, dy = nc.coverage_case(M, H, dtype, layernorm=True)
    assert not x.double().sum(-1).any()
    want_w, want_b = nc.coverage_reference(x, dy)
    assert (want_w.abs() >= M).all()
    xg, dyg = _cuda(x, dy)
    wg = torch.ones(H, dtype=dtype, device="cuda")
    bg = torch.zeros(H, dtype=dtype, device="cuda")
    _, mean, invstd = ext.layernorm_fwd(xg, wg, bg, 0.0)
    _, dw, db = ext.layernorm_bwd(xg, wg, mean, invstd, dyg)
    err = ((dw.double().cpu() - want_w).abs() / want_w.abs()).max().item()
    print(f"NORM_ROWS ln M{M} H{H} {_name(dtype)} max rel err {err:.3e}")
    assert err <= 2.0 ** -20
    assert torch.equal(db.double().cpu(), want_b)
    _, dw2, db2 = ext.layernorm_bwd(xg, wg, mean, invstd, dyg)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# -- 5. rejections: one per host check, nothing is launched ------------------------------------

ENTRIES = {
    # name: (argument names in call order, role of each tensor argument)
    "rmsnorm_fwd": (("x", "w", "eps"), {"x": "x", "w": "param"}),
    "rmsnorm_bwd": (("x", "w", "invrms", "dy"),
                    {"x": "x", "w": "param", "invrms": "stat", "dy": "like"}),
    "rmsnorm_fwd_add": (("x", "res", "w", "eps"), {"x": "x", "res": "like", "w": "param"}),
    "rmsnorm_bwd_add": (("x", "w", "invrms", "dy", "dsum"),
                        {"x": "x", "w": "param", "invrms": "stat", "dy": "like",
                         "dsum": "like"}),
    "layernorm_fwd": (("x", "w", "b", "eps"), {"x": "x", "w": "param", "b": "param"}),
    "layernorm_bwd": (("x", "w", "mean", "invstd", "dy"),
                      {"x": "x", "w": "param", "mean": "stat", "invstd": "stat",
                       "dy": "like"}),
}


def _strided(t):
    """the same values with a stride of 2 in the last dim"""
    big = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    big[..., ::2] = t
    out = big[..., ::2]
    assert not out.is_contiguous() or out.numel() <= 1
    return out


def _other_dtype(t):
    return t.float() if t.dtype == BF16 else t.to(BF16)


BAD = {
    "x": {
        "on_cpu": (lambda t: t.cpu(), "x must be on a GPU"),
        "fp16": (lambda t: t.half(), "x must be bf16 or fp32"),
        "3d": (lambda t: t[None], "2-D and contiguous"),
        "strided": (_strided, "2-D and contiguous"),
        "no_columns": (lambda t: t[:, :0], "1 <= H"),
    },
    "param": {
        "on_cpu": (lambda t: t.cpu(), "must be on x's device, in x's dtype, contiguous, with H"),
        "other_dtype": (_other_dtype, "in x's dtype, contiguous, with H"),
        "short": (lambda t: t[:-1].contiguous(), "with H = "),
        "long": (lambda t: torch.cat((t, t)), "with H = "),
        "strided": (_strided, "contiguous, with H"),
    },
    "like": {
        "on_cpu": (lambda t: t.cpu(), "in x's dtype and shape, contiguous"),
        "other_dtype": (_other_dtype, "in x's dtype and shape, contiguous"),
        "fewer_rows": (lambda t: t[:-1].contiguous(), "in x's dtype and shape, contiguous"),
        "transposed_shape": (lambda t: t.t().contiguous(), "in x's dtype and shape, contiguous"),
        "strided": (_strided, "in x's dtype and shape, contiguous"),
    },
    "stat": {
        "on_cpu": (lambda t: t.cpu(), "fp32, contiguous, with M"),
        "fp64": (lambda t: t.double(), "fp32, contiguous, with M"),
        "bf16": (lambda t: t.to(BF16), "fp32, contiguous, with M"),
        "short": (lambda t: t[:-1].contiguous(), "with M = "),
        "strided": (_strided, "fp32, contiguous, with M"),
    },
}

REJECTS = [(entry, arg, bad) for entry, (_, roles) in ENTRIES.items()
           for arg, role in roles.items() for bad in BAD[role]]


def _good_args(dtype, M=6, H=24):
    x, w, b, dy = nc.make_rows(M, H, dtype, seed=9)
    x, w, b, dy = _cuda(x, w, b, dy)
    stat = torch.ones(M, dtype=FP32, device="cuda")
    return dict(x=x, w=w, b=b, dy=dy, res=dy.clone(), dsum=dy.clone(), invrms=stat,
                mean=stat.clone(), invstd=stat.clone(), eps=1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry,arg,bad", REJECTS, ids=lambda v: str(v))
def test_rejects(entry, arg, bad, dtype):
    names, roles = ENTRIES[entry]
    args = _good_args(dtype)
    fn = getattr(hip.ext(), entry)
    fn(*[args[n] for n in names])          # the unchanged arguments are accepted
    change, msg = BAD[roles[arg]][bad]
    args[arg] = change(args[arg])
    with pytest.raises(RuntimeError, match=f"{entry}: .*{msg}"):
        fn(*[args[n] for n in names])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_no_rows_returns_empty_outputs(dtype):
    """M = 0: empty outputs, zero column sums, no launch (a 0-block grid is a
    launch error)"""
    ext = hip.ext()
    H = 24
    a = _good_args(dtype, M=0, H=H)
    y, ir = ext.rmsnorm_fwd(a["x"], a["w"], 1e-6)
    assert y.shape == (0, H) and ir.shape == (0,)
    y, s, ir = ext.rmsnorm_fwd_add(a["x"], a["res"], a["w"], 1e-6)
    assert y.shape == s.shape == (0, H) and ir.shape == (0,)
    for dx, dw in (ext.rmsnorm_bwd(a["x"], a["w"], a["invrms"], a["dy"]),
                   ext.rmsnorm_bwd_add(a["x"], a["w"], a["invrms"], a["dy"], a["dsum"])):
        assert dx.shape == (0, H) and dw.shape == (H,) and dw.dtype == FP32 and not dw.any()
    y, mean, invstd = ext.layernorm_fwd(a["x"], a["w"], a["b"], 1e-5)
    assert y.shape == (0, H) and mean.shape == invstd.shape == (0,)
    dx, dw, db = ext.layernorm_bwd(a["x"], a["w"], a["mean"], a["invstd"], a["dy"])
    assert dx.shape == (0, H) and dw.shape == db.shape == (H,)
    assert not dw.any() and not db.any()
    torch.cuda.synchronize()


# -- 6. dispatch ------------------------------------------------------------------------------------

def _spy(monkeypatch, cls):
    calls = []
    real = cls.apply

    def wrapped(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(cls, "apply", wrapped)
    return calls


def _op_inputs(x_dtype, w_dtype, strided_w=False, H=40):
    x, w, b, dy = nc.make_rows(6, H, FP32, seed=11)
    x, dy = x.to(x_dtype).cuda().view(2, 3, H), dy.to(x_dtype).cuda().view(2, 3, H)
    w, b = w.to(w_dtype).cuda(), b.to(w_dtype).cuda()
    if strided_w:
        w, b = _strided(w), _strided(b)
    return x.requires_grad_(), w.requires_grad_(), b.requires_grad_(), dy


@pytest.mark.parametrize("strided_w", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_dispatch_keeps_hip_path(dtype, strided_w, monkeypatch):
    """weight and bias in x's dtype run the kernels, through autograd, also
    when they are not contiguous; the results are those of contiguous ones"""
    calls = {c.__name__: _spy(monkeypatch, c)
             for c in (Fn._HipRMSNorm, Fn._HipAddRMSNorm, Fn._HipLayerNorm)}
    x, w, b, dy = _op_inputs(dtype, dtype, strided_w)
    xc, wc, bc, _ = _op_inputs(dtype, dtype, False)
    for op, args, ref_args in (
            (ops.rmsnorm, (x, w), (xc, wc)),
            (ops.layernorm, (x, w, b), (xc, wc, bc)),
            (lambda *a: ops.add_rmsnorm(a[0], a[0].detach(), *a[1:])[0], (x, w), (xc, wc))):
        got = torch.autograd.grad(op(*args), args, dy)
        want = torch.autograd.grad(op(*ref_args), ref_args, dy)
        for u, v in zip(got, want):
            assert u.shape == v.shape and torch.equal(u, v)
    # add_rmsnorm has the fused path in bf16 only; in fp32 it is x + res, then rmsnorm
    fused = 2 if dtype == BF16 else 0
    assert {k: len(v) for k, v in calls.items()} == {
        "_HipRMSNorm": 4 - fused, "_HipAddRMSNorm": fused, "_HipLayerNorm": 2}


@pytest.mark.parametrize("x_dtype,w_dtype", [(BF16, FP32), (FP32, BF16)])
def test_dispatch_guard_uses_torch(x_dtype, w_dtype, monkeypatch):
    """a weight in another dtype than x never reaches the kernels, which would
    read it through x's element type"""
    def no_hip(*a, **kw):
        raise AssertionError("reached the HIP norm kernels")

    for c in (Fn._HipRMSNorm, Fn._HipAddRMSNorm, Fn._HipLayerNorm):
        monkeypatch.setattr(c, "apply", no_hip)
    x, w, b, dy = _op_inputs(x_dtype, w_dtype)
    y = ops.rmsnorm(x, w, 1e-6)
    want = ops.rmsnorm_torch(x.detach(), w.detach(), 1e-6)
    assert y.dtype == want.dtype and torch.equal(y, want)
    gx, gw = torch.autograd.grad(y, (x, w), dy.to(y.dtype))
    assert gx.dtype == x_dtype and gw.dtype == w_dtype
    assert torch.isfinite(gx.float()).all() and torch.isfinite(gw.float()).all()
    normed, s = ops.add_rmsnorm(x, x.detach(), w, 1e-6)
    assert torch.equal(s, x + x) and normed.shape == x.shape
    # F.layer_norm does not mix dtypes on the GPU: the torch path answers with
    # its own error, where the kernel would have read w and b as x's type
    with pytest.raises(RuntimeError, match="expected scalar type"):
        ops.layernorm(x, w, b, 1e-5)
