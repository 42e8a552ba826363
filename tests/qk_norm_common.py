"""Float64 reference and error bounds for the per-head QK RMSNorm + RoPE
kernels, shared by tests/test_gpu_qk_norm_rope.py and tests/test_qk_norm.py.

The reference is the UNROUNDED chain rope(w * x * invrms) of one tensor
[B, heads, S, hd] and its analytic gradients; the bounds follow the project's
convention of one 2^-8 term per bf16 intermediate plus an fp32 term."""

import torch

U8, U23 = 2.0 ** -8, 2.0 ** -23


def rot_half(t):
    h = t.shape[-1] // 2
    return torch.cat((-t[..., h:], t[..., :h]), dim=-1)


def rot_half_t(t):
    """transpose of rot_half: what the backward rotation applies"""
    h = t.shape[-1] // 2
    return torch.cat((t[..., h:], -t[..., :h]), dim=-1)


def reference(x, w, dy, cos, sin, eps):
    """x, dy: [B, heads, S, hd]; w: [hd]; cos, sin: [>=S, hd].  Everything is
    taken to float64.  Returns a dict with the outputs, the gradients and the
    magnitudes the bounds are built from."""
    x, w, dy = x.double().cpu(), w.double().cpu(), dy.double().cpu()
    S, hd = x.shape[-2], x.shape[-1]
    c, s = cos[:S].double().cpu(), sin[:S].double().cpu()
    ir = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    nhat = x * ir
    y = w * nhat
    out = y * c + rot_half(y) * s
    out_mag = y.abs() * c.abs() + rot_half(y).abs() * s.abs()
    # backward
    g = dy * c + rot_half_t(dy * s)
    g_mag = dy.abs() * c.abs() + rot_half_t(dy * s).abs()
    dn = g * w
    m = (dn * nhat).mean(-1, keepdim=True)
    dx = ir * (dn - nhat * m)
    dn_mag = g_mag * w.abs()
    dx_mag = ir * (dn_mag + nhat.abs() * (dn_mag * nhat.abs()).mean(-1, keepdim=True))
    dw = (g * nhat).sum(dim=(0, 1, 2))
    dw_mag = (g_mag * nhat.abs()).sum(dim=(0, 1, 2))
    rows = x.shape[0] * x.shape[1] * x.shape[2]
    return dict(
        out=out, invrms=ir.squeeze(-1), dx=dx, dw=dw,
        # three bf16 intermediates (n, y, out), fp32 sums of hd terms behind invrms
        out_bound=(3 * U8 + hd * U23) * out_mag,
        # dx is rounded once; g, nhat, dn and the row mean are fp32
        dx_bound=U8 * dx.abs() + hd * U23 * dx_mag,
        # fp32 accumulation over the rows, no bf16 anywhere
        dw_bound=rows * U23 * dw_mag,
    )


def worst_fraction(got, ref, bound):
    """max of |got - ref| / bound; an error where the bound is 0 counts as inf"""
    err = (got.double().cpu() - ref).abs()
    frac = torch.where(err == 0, torch.zeros_like(err),
                       err / bound.clamp_min(1e-300))
    return frac.max().item()


def make_case(B, heads, S, hd, seed, zero_row=True):
    """bf16 x with row scales spread over 2^-6..2^6 (so eps matters in some
    rows and not in others) and one all-zero row, weights 1 + 0.5 randn, dy
    randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, heads, S, hd, generator=g)
    scale = 2.0 ** torch.randint(-6, 7, (B, heads, S, 1), generator=g).float()
    x = (x * scale).to(torch.bfloat16)
    if zero_row:
        x[B - 1, heads - 1, S // 2] = 0
    w = (1 + 0.5 * torch.randn(hd, generator=g)).to(torch.bfloat16)
    dy = torch.randn(B, heads, S, hd, generator=g).to(torch.bfloat16)
    return x, w, dy


def in_layout(t, layout):
    """[B, h, S, hd] values as BHSD-contiguous ("bhsd") or as the transposed
    view of a BSHD buffer ("bshd")"""
    if layout == "bhsd":
        return t.contiguous()
    return t.transpose(1, 2).contiguous().transpose(1, 2)
