"""Shared helpers for the intra-document masking tests (CPU only, importable
without a GPU): `doc_start` builders, inputs, the masked float64 reference
and the masked bf16 emulation.

Convention under test: `doc_start` is int32 [B, S]; doc_start[b, i] is the
index of the first token of the document token i belongs to, and query i
attends to kv j iff doc_start[b, i] <= j <= i, for every head.  Bounds are
the project's, from attn_variant_worker: `all_ratios` (tol 2e-2 for out,
3e-2 for dq/dk/dv) and `LSE_TOL` (1e-2 absolute), against float64 on the CPU.
"""

import torch

import attn_variant_worker as aw
import gqa_common as gc

B, NH = 2, 4
# dout is gqa_common's (magnitude 0.5) halved again: with q at Q_GAIN the dK
# error of the bf16 emulation (dS rounding times |q|) measured 0.69 of the
# bound at 0.5 and 0.39 at 0.25; the inputs keep a 2x headroom rather than
# the bound being widened
DOUT_SCALE = 0.5
Q_GAIN = 4.0   # q of every second document is scaled by this


def doc_start_from_lengths(rows, S):
    """int32 [B, S] from one list of document lengths per batch row."""
    out = torch.empty(len(rows), S, dtype=torch.int32)
    for b, lengths in enumerate(rows):
        assert sum(lengths) == S and min(lengths) >= 1, (lengths, S)
        pos = 0
        for n in lengths:
            out[b, pos:pos + n] = pos
            pos += n
    return out


def is_well_formed(ds):
    """the three properties the kernels rely on"""
    ds = ds.long()
    pos = torch.arange(ds.shape[-1]).expand_as(ds)
    return bool((ds[..., 1:] >= ds[..., :-1]).all() and (ds <= pos).all()
                and (ds >= 0).all() and (torch.gather(ds, -1, ds) == ds).all())


def allowed(ds):
    """bool [B, 1, S, S]: True where query i may attend to kv j"""
    S = ds.shape[-1]
    pos = torch.arange(S)
    i, j = pos[:, None], pos[None, :]
    return ((j <= i) & (j >= ds.long()[:, :, None])).unsqueeze(1)


# The boundary grid at S = 320 (two forward q blocks of 256, the second
# partial; five kv tiles of 64).  One list of document lengths per batch row;
# the two rows always differ.
S_GRID = 320
GRID = {
    # a boundary in the middle of a 32-subtile; row 1 is a single document
    "mid45": ([45, 275], [320]),
    # boundaries exactly on 32, 64 and 256
    "on_32_64_256": ([32, 32, 192, 64], [64, 192, 64]),
    # a document that begins at 256: the second q block skips kv tiles 0..3
    # and the first kv block's q loop ends after q tile 3
    "start256": ([256, 64], [128, 128, 64]),
    # a boundary at 300, inside the second q block: its waves differ in ds
    "b300": ([300, 20], [150, 150, 20]),
    # a run of five one-token documents: out[i] == v[i], lse[i] == s_ii
    "ones5": ([100, 1, 1, 1, 1, 1, 215], [30, 1, 1, 1, 1, 1, 285]),
    # one row with a single document, the other split in the middle
    "single": ([320], [160, 160]),
}
ONES5_ROWS = (range(100, 105), range(30, 35))   # per batch row
SHORT = {80: ([50, 30], [80]), 33: ([20, 13], [1, 32])}


def grid_doc_start(name):
    return doc_start_from_lengths(GRID[name], S_GRID)


def make_inputs(nkv, S, hd, ds, seed=0):
    """gqa_common.make_inputs with q scaled by 1x and Q_GAIN on alternating
    documents, so that a leak across a boundary moves the result by far more
    than the bound."""
    q, k, v, dout = gc.make_inputs(B, NH, nkv, S, hd, seed=seed)
    starts = (ds.long() == torch.arange(S)).long()          # [B, S]
    doc_idx = starts.cumsum(-1) - 1
    gain = torch.where(doc_idx % 2 == 1, Q_GAIN, 1.0)[:, None, :, None]
    q = (q.float() * gain).to(torch.bfloat16)
    return q, k, v, (dout.float() * DOUT_SCALE).to(torch.bfloat16)


def _scores64(q, k, ds, scale):
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    return s.masked_fill(~allowed(ds), float("-inf"))


def ref_doc(q, k, v, dout, ds, scale=None):
    """float64 masked attention on the CPU with K/V expanded by
    repeat_interleave; dK/dV summed back over each group in float64."""
    nh, nkv = q.shape[1], k.shape[1]
    hd = q.shape[-1]
    scale = hd ** -0.5 if scale is None else scale
    qd = q.detach().cpu().double().requires_grad_(True)
    kd = gc.expand_kv(k.detach().cpu(), nh).double().requires_grad_(True)
    vd = gc.expand_kv(v.detach().cpu(), nh).double().requires_grad_(True)
    s = (qd @ kd.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed(ds.cpu()), float("-inf"))
    o = torch.softmax(s, -1) @ vd
    o.backward(dout.detach().cpu().double())
    return {"o": o.detach(), "lse": torch.logsumexp(s, -1).detach(), "dq": qd.grad,
            "dk": gc.group_sum(kd.grad, nkv), "dv": gc.group_sum(vd.grad, nkv)}


def emulate_doc_bf16(q, k, v, dout, ds, scale=None):
    """attn_variant_worker.emulate_bf16 with the document mask: exact
    arithmetic with the kernels' bf16 roundings of P, dS and the outputs;
    the group sum as in gqa_common.emulate_gqa."""
    nh, nkv = q.shape[1], k.shape[1]
    hd = q.shape[-1]
    scale = hd ** -0.5 if scale is None else scale
    rnd = lambda x: x.to(torch.bfloat16).double()   # noqa: E731
    qd, dod = q.double(), dout.double()
    kd, vd = gc.expand_kv(k, nh).double(), gc.expand_kv(v, nh).double()
    s = _scores64(q, gc.expand_kv(k, nh), ds, scale)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = rnd((rnd(p) @ vd) / l)
    lse = (m + torch.log(l)).squeeze(-1)
    pn = torch.exp(s - lse[..., None])
    delta = (dod * o).sum(-1, keepdim=True)
    dsc = rnd(pn * (dod @ vd.transpose(-1, -2) - delta) * scale)
    return {"o": o, "lse": lse, "dq": rnd(dsc @ kd),
            "dk": rnd(gc.group_sum(rnd(dsc.transpose(-1, -2) @ qd), nkv)),
            "dv": rnd(gc.group_sum(rnd(rnd(pn).transpose(-1, -2) @ dod), nkv))}


def gpu_cases():
    """(id, nkv, S, hd, doc_start) of every kernel case of
    tests/test_gpu_attention_docmask.py's value tests."""
    out = []
    for name in GRID:
        for hd in (64, 40):
            for nkv in (4, 2):
                out.append((f"{name}-hd{hd}-nkv{nkv}", nkv, S_GRID, hd, grid_doc_start(name)))
    for S, rows in SHORT.items():
        out.append((f"S{S}-hd64-nkv2", 2, S, 64, doc_start_from_lengths(rows, S)))
    return out


def run_kernels(ext, q, k, v, dout, ds, scale=None):
    """attn_fwd + attn_bwd with doc_start on the inputs' own device/layout"""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = ext.attn_fwd(q, k, v, scale, ds)
    dq, dk, dv = ext.attn_bwd(q, k, v, o, lse, dout, scale, ds)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
