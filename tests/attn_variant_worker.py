"""Shared helpers for tests/test_gpu_attention_edges.py, and the child-process
worker for its variant tests.

Helpers (CPU only, importable without a GPU):
  * structured q/k/v/dout that drive the v3 forward's rescale branch with
    non-zero accumulators (`make_structured`),
  * an emulation of the forward's wave-wide defer-max decision on float64
    scores, used to assert that the inputs really hit the branch
    (`rescale_jumps`, `check_structured_conditions`),
  * the float64 reference and a bf16-emulated float64 result
    (`ref_attention`, `emulate_bf16`),
  * the project's per-element bound as a ratio (`bound_ratio`; <= 1 passes).

Worker: the RELORA_AMD_ATTN_* / RELORA_AMD_DQ_* flags are read once per
process into function-local statics, so each variant needs a fresh process.
`python tests/attn_variant_worker.py [--hd128]` runs a short case list
through `attn_fwd`/`attn_bwd` under whatever flags its environment carries
and prints one JSON line of max errors; the parent test asserts the bounds.
"""

import json
import math
import os
import sys

import torch

# per-element bound of assert_close_bf16: err <= atol + rtol * max(1, |ref|)
FWD_TOL = 2e-2    # atol = rtol, forward output
GRAD_TOL = 3e-2   # atol = rtol, dq / dk / dv
LSE_TOL = 1e-2    # absolute

LOG2E = 1.4426950408889634
DEFER_MAX_THR = 11.5   # attention.hip: log2-domain defer-max threshold
WAVE_ROWS = 32         # q rows per wave in the v3 forward
SUBTILE = 32           # kv rows per online-softmax update

# Structured-input constants.  q = 0.5*randn + gain_i * ones(hd),
# k = 0.5*randn + ramp_j * ones(hd)/sqrt(hd), so that the scaled score is
# gain_i * ramp_j + noise at every hd (at hd=64 this is the e = ones/8
# construction: q = .. + gain*8*e, k = .. + ramp*e).
HOT_GAIN = 12.0        # rows i % 32 == 0 of the "rescale"/"descending" sets
RESCALE_RAMP = 1.0     # ramp_j = RESCALE_RAMP * (j // 32)
# Tuned on the CPU over steps 0.45 .. 0.6: with no rescale after the first
# subtile the running max stays stale, so the excess accumulates over the
# 10 subtiles of S=320 and the step has to keep the total under 11.5.
# Measured largest excess at 0.6: hd32 9.62, hd64 9.04, hd128 9.49 (0.45
# gave 7.4 .. 7.7).
DEFER_RAMP = 0.6
# Magnitudes of v and dout.  Measured worst bf16-emulation error over the
# three sets x hd {32, 64, 128}, as a fraction of the per-element bound
# (must stay <= 0.5): forward 0.126 (max abs err 0.0077, |o| up to 3.6),
# lse 0, dq 0.049, dk 0.479 (descending, hd128), dv 0.116.  With dout at
# magnitude 1 the backward emulation misses the headroom (dk about twice
# the above: dS rounding times the hot rows' q = 12), so dout is halved
# rather than the bound widened.
V_MAG = 1.0
DOUT_MAG = 0.5

# Generator seeds per hd, searched on the CPU (scores only, no kernel
# involved) so that the "rescale" set meets check_structured_conditions:
# a hot row is the first row of its wave and sees a single key of the
# wave's last (diagonal) subtile, so whether that last jump passes the
# threshold is up to the noise; wave 1 has no other subtile to rescale at
# and wave 2 needs it for its second, in both heads.  That makes passing
# seeds rare (about 1 in 5000).  To repeat the search after changing S, nh
# or a constant above: `python tests/attn_variant_worker.py --search-seeds`
# (find_structured_seed below; a few minutes of CPU), and copy its output.
STRUCTURED_SEED = {32: 5648, 64: 8210, 128: 17462}

STRUCTURED_KINDS = ("rescale", "deferred", "descending")


def make_structured(kind, hd, S=320, nh=2, seed=None):
    """bf16 CPU tensors q, k, v, dout of shape [1, nh, S, hd]."""
    assert kind in STRUCTURED_KINDS
    seed = STRUCTURED_SEED[hd] if seed is None else seed
    g = torch.Generator().manual_seed(1000 + seed)
    ones = torch.ones(hd, dtype=torch.float64)
    grp = (torch.arange(S) // SUBTILE).double()
    if kind == "rescale":
        ramp = RESCALE_RAMP * grp
    elif kind == "descending":
        ramp = RESCALE_RAMP * (grp.max() - grp)
    else:
        ramp = DEFER_RAMP * grp
    gain = torch.ones(S, dtype=torch.float64)
    if kind != "deferred":
        gain[torch.arange(S) % WAVE_ROWS == 0] = HOT_GAIN

    def rn():
        return torch.randn(1, nh, S, hd, generator=g, dtype=torch.float64)

    q = 0.5 * rn() + gain[None, None, :, None] * ones
    k = 0.5 * rn() + ramp[None, None, :, None] * ones / math.sqrt(hd)
    v = V_MAG * rn()
    dout = DOUT_MAG * rn()
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, dout))


def hot_row_mask(S):
    return torch.arange(S) % WAVE_ROWS == 0


def _scores64(q, k, scale):
    S = q.shape[-2]
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    return s.masked_fill(mask, float("-inf"))


def rescale_jumps(q, k, scale=None):
    """Replay the v3 forward's defer-max policy on float64 scores.

    Each 32-row wave walks the 32-kv subtiles up to its diagonal.  A lane's
    jump is (subtile max - running max) in the log2 domain; the wave
    rescales, every lane to its own new max, when any lane's jump passes
    DEFER_MAX_THR (or at the first subtile).  Returns jumps[.., S, n_sub]
    with NaN where a subtile is not visited or is the first, and the
    boolean fired[.., S // 32 (ceil), n_sub].
    """
    hd = q.shape[-1]
    scale = hd ** -0.5 if scale is None else scale
    s2 = _scores64(q, k, scale) * LOG2E
    S = s2.shape[-1]
    n_sub = (S + SUBTILE - 1) // SUBTILE
    n_wave = (S + WAVE_ROWS - 1) // WAVE_ROWS
    lead = s2.shape[:-2]
    jumps = torch.full(lead + (S, n_sub), float("nan"), dtype=torch.float64)
    fired = torch.zeros(lead + (n_wave, n_sub), dtype=torch.bool)
    for w in range(n_wave):
        r0, r1 = w * WAVE_ROWS, min((w + 1) * WAVE_ROWS, S)
        m2 = torch.full(lead + (r1 - r0,), float("-inf"), dtype=torch.float64)
        for t in range(n_sub):
            if t * SUBTILE > r1 - 1:
                break
            m_tile = s2[..., r0:r1, t * SUBTILE:(t + 1) * SUBTILE].amax(-1)
            if t == 0:
                m2 = m_tile
                continue
            jump = m_tile - m2
            jumps[..., r0:r1, t] = jump
            fire = (jump > DEFER_MAX_THR).any(-1)
            fired[..., w, t] = fire
            m2 = torch.where(fire[..., None], torch.maximum(m2, m_tile), m2)
    return jumps, fired


def check_structured_conditions(kind, q, k):
    """Assert that the inputs reach the branch they are built for; returns
    the measured figures.  Pure CPU."""
    jumps, _ = rescale_jumps(q, k)
    S = q.shape[-2]
    hot = hot_row_mask(S)
    over = jumps > DEFER_MAX_THR          # NaN compares False
    stats = {"max_jump": float(jumps.nan_to_num(float("-inf")).max())}
    if kind == "rescale":
        n_over = over.sum(-1)             # [1, nh, S]
        n_wave = S // WAVE_ROWS
        # Causality: wave 0 visits one subtile and wave 1 two, so "two or
        # more rescales after the first subtile" can only be asked of the
        # waves from rows 64 on; wave 1 has one such subtile and must
        # rescale there, wave 0 has none.
        for w in range(1, n_wave):
            need = min(2, w)
            rows = slice(w * WAVE_ROWS, (w + 1) * WAVE_ROWS)
            hot_ok = (n_over[..., rows][..., hot[rows]] >= need).any(-1)
            assert hot_ok.all(), f"wave {w}: no hot row with >= {need} rescales"
        cold_over = over[..., ~hot, :]
        assert not cold_over.any(), "a cold row passes the threshold"
        cold = jumps[..., ~hot, :]
        mid = ((cold > 2.0) & (cold <= DEFER_MAX_THR)).sum()
        assert mid >= 100, f"only {int(mid)} cold steps with growth in (2, 11.5]"
        stats.update(hot_over=int(over[..., hot, :].sum()),
                     hot_max=float(jumps[..., hot, :].nan_to_num(-1e9).max()),
                     cold_max=float(cold.nan_to_num(-1e9).max()),
                     cold_mid=int(mid))
    elif kind == "deferred":
        assert not over.any(), f"a jump passes the threshold: {stats['max_jump']}"
        assert stats["max_jump"] > 6.0, stats["max_jump"]
    else:  # descending: the max comes first and stays
        assert not over.any(), f"a jump passes the threshold: {stats['max_jump']}"
        assert stats["max_jump"] < 2.0, stats["max_jump"]
    return stats


def find_structured_seed(hd, S=320, nh=2, limit=20000):
    """First seed whose "rescale" set meets check_structured_conditions, and
    whose bf16 emulation keeps the 2x headroom; None if there is none below
    `limit`.  This is how STRUCTURED_SEED was filled: after changing S, nh
    or a constant above, run `python tests/attn_variant_worker.py
    --search-seeds` (CPU only, no kernel involved) and copy the result."""
    for seed in range(limit):
        q, k, v, dout = make_structured("rescale", hd, S=S, nh=nh, seed=seed)
        try:
            check_structured_conditions("rescale", q, k)
        except AssertionError:
            continue
        emu = all_ratios(emulate_bf16(q, k, v, dout), ref_attention(q, k, v, dout))
        if emu.pop("lse") <= LSE_TOL / 2 and max(emu.values()) <= 0.5:
            return seed
    return None


def ref_attention(q, k, v, dout=None, scale=None):
    """Plain float64 causal softmax attention on the CPU, from the given
    (bf16) inputs upcast; autograd backward when dout is given."""
    hd = q.shape[-1]
    scale = hd ** -0.5 if scale is None else scale
    qd, kd, vd = (t.detach().cpu().double().requires_grad_(dout is not None)
                  for t in (q, k, v))
    S = qd.shape[-2]
    s = (qd @ kd.transpose(-1, -2)) * scale
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), 1)
    s = s.masked_fill(mask, float("-inf"))
    o = torch.softmax(s, -1) @ vd
    res = {"o": o.detach(), "lse": torch.logsumexp(s, -1).detach()}
    if dout is not None:
        o.backward(dout.detach().cpu().double().expand_as(o))
        res.update(dq=qd.grad, dk=kd.grad, dv=vd.grad)
    return res


def _bf16_round(x):
    return x.to(torch.bfloat16).double()


def emulate_bf16(q, k, v, dout, scale=None):
    """What an exact-arithmetic kernel with the kernels' bf16 roundings would
    give: P (forward: against the row max; backward: normalised) and dS are
    rounded to bf16 before their second matmul, the outputs to bf16, and
    delta uses the bf16 forward output."""
    hd = q.shape[-1]
    scale = hd ** -0.5 if scale is None else scale
    qd, kd, vd, dod = (t.double() for t in (q, k, v, dout))
    s = _scores64(q, k, scale)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = _bf16_round((_bf16_round(p) @ vd) / l)
    lse = (m + torch.log(l)).squeeze(-1)
    pn = torch.exp(s - lse[..., None])
    delta = (dod * o).sum(-1, keepdim=True)
    ds = _bf16_round(pn * (dod @ vd.transpose(-1, -2) - delta) * scale)
    return {
        "o": o, "lse": lse,
        "dq": _bf16_round(ds @ kd),
        "dk": _bf16_round(ds.transpose(-1, -2) @ qd),
        "dv": _bf16_round(_bf16_round(pn).transpose(-1, -2) @ dod),
    }


def bound_ratio(got, ref, tol):
    """max over elements of err / (tol + tol * max(1, |ref|)); the
    assert_close_bf16 bound holds iff this is <= 1.  NaN/inf give inf."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    return float((err / (tol + tol * ref.abs().clamp_min(1.0))).max())


def grad_ratios(got, ref, rows=None):
    """bound ratios of a kernel result dict/tuple against ref_attention's."""
    sel = (lambda t: t) if rows is None else (lambda t: t[..., rows, :])
    return {n: bound_ratio(sel(got[n]), sel(ref[n]), GRAD_TOL)
            for n in ("dq", "dk", "dv")}


def strided_qkv(B, nh, S, hd, seed=0, device="cpu", n=3):
    """n tensors [B, nh, S, hd] that are transposed views of BSHD buffers —
    the layout the models hand to flash_attention."""
    g = torch.Generator().manual_seed(2000 + seed)
    bufs = [torch.randn(B, S, nh * hd, generator=g).to(torch.bfloat16).to(device)
            for _ in range(n)]
    return [b.view(B, S, nh, hd).transpose(1, 2) for b in bufs]


def run_kernels(ext, q, k, v, dout, scale=None):
    """attn_fwd + attn_bwd on the inputs' own device and layout."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = ext.attn_fwd(q, k, v, scale)
    dq, dk, dv = ext.attn_bwd(q, k, v, o, lse, dout, scale)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def all_ratios(got, ref):
    r = {"o": bound_ratio(got["o"], ref["o"], FWD_TOL),
         "lse": float((got["lse"].detach().cpu().double() - ref["lse"]).abs().max())}
    if not math.isfinite(r["lse"]):
        r["lse"] = float("inf")
    r.update(grad_ratios(got, ref))
    return r


def worker_cases(hd128):
    """(name, q, k, v, dout) on the CPU for the variant children."""
    cases = [("rescale_hd64",) + make_structured("rescale", 64)]
    sq, sk, sv, sdo = strided_qkv(2, 3, 160, 64, n=4)
    cases.append(("strided_hd64", sq, sk, sv, sdo))
    hds = (32, 64, 128) if hd128 else (32, 64)
    for S in (33, 257):
        for hd in hds:
            g = torch.Generator().manual_seed(3000 + S + hd)
            cases.append((f"S{S}_hd{hd}",) + tuple(
                torch.randn(1, 2, S, hd, generator=g).to(torch.bfloat16)
                for _ in range(4)))
    if hd128:
        cases.append(("rescale_hd128",) + make_structured("rescale", 128))
    return cases


def main(argv):
    if "--search-seeds" in argv:
        print({hd: find_structured_seed(hd) for hd in sorted(STRUCTURED_SEED)})
        return
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd.ops import hip

    ext = hip.ext()
    assert ext is not None, "HIP extension not built"
    assert torch.cuda.is_available(), "variant worker needs a GPU"
    out = {}
    for name, q, k, v, dout in worker_cases("--hd128" in argv):
        ref = ref_attention(q, k, v, dout)
        got = run_kernels(ext, *(t.cuda() for t in (q, k, v, dout)))
        torch.cuda.synchronize()
        out[name] = all_ratios(got, ref)
    print("ATTN_VARIANT_RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
