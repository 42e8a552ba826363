"""swiglu.hip (SwiGLU, exact-erf GELU, forward and backward) against float64.

Exhaustive over bf16: every bit pattern that is zero or a finite normal number,
65026 of the 65536, goes in as g (SwiGLU) and as x (GELU) in one launch each,
against u in {1, -3, 2^-20, 2^20} and dy in {1, -0.5}.  The 256 inf/NaN
patterns and the 254 subnormals, 510 of 65536, are left out; that share is a
condition of this test.  The references g * sigmoid(g) * u, x * Phi(x) and
their derivatives, the bounds (one 2^-8 * |ref| for the rounding of the
output, an absolute term of 4 times the CPU-measured error of the same fp32
formulas, 2^-126 for underflow) and the measured multiples are in
tests/norm_common.py.

Finite results: __expf(-g) overflows to inf for g < -88 and the quotient must
still be a zero, not a NaN.  Every output whose float64 reference a bf16 can
hold must be finite and inside its bound.  g * sigmoid(g) * u itself leaves
the bf16 range at the top of the sweep for u = 2^20 and u = -3; there the
rounded result is an infinity of the reference's sign, and that (or the
largest finite values) is what is required.

The fp32 instantiation runs the same functions on a 4096-point grid over
[-20, 20] and at +-88, +-100 and +-1e4.  Lengths: 1, 7 (tail only), 8, 9,
2047, 2048 * 8 + 3 (one vector per thread of 8 blocks, and a tail) and
2048 * 256 * 8 + 8 * 5 + 3: five vectors and a tail beyond what the capped grid
of 2048 blocks of 256 threads covers in one grid-stride pass."""

import pytest
import torch

import norm_common as nc
from relora_amd.ops import hip

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
OUTPUTS = ("swiglu_y", "swiglu_dg", "swiglu_du", "gelu_y", "gelu_dx")


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _poison(n, dtype):
    """make the block the next output of n elements most likely lands in hold
    NaN, so an element the kernel skips is seen"""
    t = torch.full((n,), float("nan"), dtype=dtype, device="cuda")
    del t


def _run(g, u, dy):
    ext = hip.ext()
    n, dtype = g.numel(), g.dtype
    out = {}
    _poison(n, dtype)
    out["swiglu_y"] = ext.swiglu_fwd(g, u)
    _poison(n, dtype)
    _poison(n, dtype)
    out["swiglu_dg"], out["swiglu_du"] = ext.swiglu_bwd(g, u, dy)
    _poison(n, dtype)
    out["gelu_y"] = ext.gelu_fwd(g)
    _poison(n, dtype)
    out["gelu_dx"] = ext.gelu_bwd(g, dy)
    torch.cuda.synchronize()
    for v in out.values():
        assert v.shape == g.shape and v.dtype == dtype
    return out


def _check(tag, g, u, dy, got):
    ref, unit = nc.act_reference(g.cpu(), u.cpu(), dy.cpu())
    bound = nc.act_bounds(ref, unit, g.dtype)
    worst = {}
    for k in OUTPUTS:
        o = got[k].double().cpu()
        assert not torch.isnan(o).any(), (tag, k)
        fits = ref[k].abs() <= nc.BF16_MAX
        assert torch.isfinite(o[fits]).all(), (tag, k)
        worst[k] = nc.worst_fraction(o[fits], ref[k][fits], bound[k][fits])
        over = ~fits
        if over.any():
            assert g.dtype == BF16 and k == "swiglu_y", (tag, k)
            assert (torch.sign(o[over]) == torch.sign(ref[k][over])).all(), (tag, k)
            assert (o[over].abs() >= nc.BF16_MAX * (1 - 2.0 ** -6)).all(), (tag, k)
    print(f"ACT_FRAC {tag} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


# -- 1. exhaustive over bf16, fp32 grid ---------------------------------------------

@pytest.mark.parametrize("dy", nc.SWEEP_DY)
@pytest.mark.parametrize("u", nc.SWEEP_U)
def test_bf16_exhaustive(u, dy):
    g = nc.bf16_sweep().cuda()
    assert g.numel() == 65536 - 510 and torch.isfinite(g.float()).all()
    uu, dd = torch.full_like(g, u), torch.full_like(g, dy)
    assert uu[0].item() == u and dd[0].item() == dy      # representable in bf16
    _check(f"bf16 u={u} dy={dy}", g, uu, dd, _run(g, uu, dd))


@pytest.mark.parametrize("dy", nc.SWEEP_DY)
@pytest.mark.parametrize("u", nc.SWEEP_U)
def test_fp32_grid(u, dy):
    g = nc.fp32_grid().cuda()
    uu, dd = torch.full_like(g, u), torch.full_like(g, dy)
    _check(f"fp32 u={u} dy={dy}", g, uu, dd, _run(g, uu, dd))


# -- 2. lengths -----------------------------------------------------------------------

LENGTHS = [1, 7, 8, 9, 2047, 2048 * 8 + 3, 2048 * 256 * 8 + 8 * 5 + 3]


def _indexed(n, dtype):
    """values that change with the index, all exactly representable in bf16:
    g = ((i % 251) - 125) / 16, u = 1 + (i % 127) / 128, dy = 1 - (i % 61) / 64;
    the three periods are coprime to each other and to 8 and 256, so no two
    vectors, threads or blocks of a pass see the same triple"""
    i = torch.arange(n)
    g = ((i % 251) - 125).float() / 16
    u = 1 + (i % 127).float() / 128
    dy = 1 - (i % 61).float() / 64
    for t in (g, u, dy):
        assert torch.equal(t.to(BF16).float(), t)
    return g.to(dtype).cuda(), u.to(dtype).cuda(), dy.to(dtype).cuda()


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(n, dtype):
    g, u, dy = _indexed(n, dtype)
    got = _run(g, u, dy)
    _check(f"{_name(dtype)} n={n}", g, u, dy, got)
    # the vector part does not depend on the tail: bit-equal to the same
    # kernel on the 8-aligned prefix alone
    n8 = n // 8 * 8
    alone = _run(g[:n8], u[:n8], dy[:n8])
    for k in OUTPUTS:
        assert torch.equal(got[k][:n8], alone[k]), (k, n)


def test_shape_is_kept():
    g, u, dy = _indexed(3 * 5 * 7, BF16)
    g, u, dy = (t.view(3, 5, 7) for t in (g, u, dy))
    got = _run(g, u, dy)
    flat = _run(g.view(-1), u.view(-1), dy.view(-1))
    for k in OUTPUTS:
        assert got[k].shape == (3, 5, 7) and torch.equal(got[k].view(-1), flat[k])


# -- 3. rejections: one per host check, nothing is launched --------------------------------

ENTRIES = {
    "swiglu_fwd": (("g", "u"), {"g": "first", "u": "same"}),
    "swiglu_bwd": (("g", "u", "dy"), {"g": "first", "u": "same", "dy": "same"}),
    "gelu_fwd": (("g",), {"g": "first"}),
    "gelu_bwd": (("g", "dy"), {"g": "first", "dy": "same"}),
}


def _strided(t):
    big = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    big[::2] = t
    return big[::2]


BAD = {
    "first": {
        "on_cpu": (lambda t: t.cpu(), "must be on a GPU"),
        "fp16": (lambda t: t.half(), "must be bf16 or fp32"),
        "strided": (_strided, "must be contiguous"),
    },
    "same": {
        "on_cpu": (lambda t: t.cpu(), "on the first argument's device"),
        "other_dtype": (lambda t: t.float() if t.dtype == BF16 else t.to(BF16),
                        "in its dtype"),
        "shorter": (lambda t: t[:-1].contiguous(), "with as many elements"),
        "longer": (lambda t: torch.cat((t, t)), "with as many elements"),
        "strided": (_strided, "contiguous, with as many elements"),
    },
}

REJECTS = [(entry, arg, bad) for entry, (_, roles) in ENTRIES.items()
           for arg, role in roles.items() for bad in BAD[role]]


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("entry,arg,bad", REJECTS, ids=lambda v: str(v))
def test_rejects(entry, arg, bad, dtype):
    names, roles = ENTRIES[entry]
    g, u, dy = _indexed(40, dtype)
    args = dict(g=g, u=u, dy=dy)
    fn = getattr(hip.ext(), entry)
    fn(*[args[n] for n in names])          # the unchanged arguments are accepted
    change, msg = BAD[roles[arg]][bad]
    args[arg] = change(args[arg])
    with pytest.raises(RuntimeError, match=f"{entry}: .*{msg}"):
        fn(*[args[n] for n in names])


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
def test_no_elements_returns_empty_outputs(dtype):
    ext = hip.ext()
    e = torch.empty(0, 16, dtype=dtype, device="cuda")
    assert ext.swiglu_fwd(e, e).shape == (0, 16)
    dg, du = ext.swiglu_bwd(e, e, e)
    assert dg.shape == du.shape == (0, 16)
    assert ext.gelu_fwd(e).shape == (0, 16) and ext.gelu_bwd(e, e).shape == (0, 16)
    torch.cuda.synchronize()
