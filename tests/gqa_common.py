"""Shared helpers for the grouped-query attention tests (CPU only, importable
without a GPU): inputs, the float64 reference and the bf16 emulation.

Convention under test: with nh query heads and nkv kv heads, n_rep = nh // nkv
and query head h reads kv head h // n_rep (`repeat_interleave` on the head
axis, HF's `repeat_kv`), not h % nkv.
"""

import torch

import attn_variant_worker as aw

DOUT_MAG = 0.5


def make_inputs(B, nh, nkv, S, hd, seed=0):
    """bf16 CPU q [B,nh,S,hd], k, v [B,nkv,S,hd], dout [B,nh,S,hd]: independent
    randn per head, so a wrong head mapping cannot pass."""
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * nkv + S + hd)
    q = torch.randn(B, nh, S, hd, generator=g)
    k = torch.randn(B, nkv, S, hd, generator=g)
    v = torch.randn(B, nkv, S, hd, generator=g)
    dout = DOUT_MAG * torch.randn(B, nh, S, hd, generator=g)
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, dout))


def expand_kv(t, nh):
    return t.repeat_interleave(nh // t.shape[1], dim=1)


def group_sum(t, nkv):
    """[B, nh, S, hd] -> [B, nkv, S, hd], summing each group of n_rep heads."""
    B, nh, S, hd = t.shape
    return t.reshape(B, nkv, nh // nkv, S, hd).sum(2)


def ref_gqa(q, k, v, dout):
    """float64 causal attention with K/V expanded by repeat_interleave; dK/dV
    summed back over each group in float64."""
    nh, nkv = q.shape[1], k.shape[1]
    ref = aw.ref_attention(q, expand_kv(k.cpu(), nh), expand_kv(v.cpu(), nh), dout)
    ref["dk"] = group_sum(ref["dk"], nkv)
    ref["dv"] = group_sum(ref["dv"], nkv)
    return ref


def emulate_gqa(q, k, v, dout):
    """aw.emulate_bf16 per query head; the group sum of dK/dV is taken over
    the per-head bf16-rounded values and rounded again (the kernels round
    once, after an fp32 sum, so this is the more pessimistic of the two)."""
    nh, nkv = q.shape[1], k.shape[1]
    emu = aw.emulate_bf16(q, expand_kv(k, nh), expand_kv(v, nh), dout)
    emu["dk"] = group_sum(emu["dk"], nkv).to(torch.bfloat16).double()
    emu["dv"] = group_sum(emu["dv"], nkv).to(torch.bfloat16).double()
    return emu


def failures(r):
    """names of the figures of aw.all_ratios that miss the project's bounds"""
    return [n for n, x in r.items()
            if not (x <= (aw.LSE_TOL if n == "lse" else 1.0))]


def to_layout(t, transposed):
    """same values, BHSD-contiguous or the transposed view of a BSHD buffer"""
    if not transposed:
        return t.contiguous()
    return t.transpose(1, 2).contiguous().transpose(1, 2)
