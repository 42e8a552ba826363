"""Functional compute ops with HIP/CDNA4 dispatch.

Each op has two implementations:

* a hand-written gfx950 HIP kernel (``relora_amd/ops/csrc``, loaded via
  :mod:`relora_amd.ops.hip`) — the production path on MI355X;
* a pure-PyTorch implementation — the CPU path and the numerics oracle the
  kernels are tested against (tests/test_ops_*.py).

Kernel inventory parity: K1/K2 `lora_linear` (fused LoRA
GEMM), K3 `flash_attention`, K4 `rope`, K5 `rmsnorm`, K6 `layernorm`,
K7 `swiglu`, K10 `fused_cross_entropy` (chunked; never materializes *fp32*
logits — row stats and the in-place grad are fp32-accurate HIP kernels over
bf16 logit chunks. The default single-chunk config does hold one full
[M,V] bf16 logits buffer (~1.6 GB at the flagship shape — cheap against
288 GB HBM); set RELORA_AMD_CE_CHUNK lower to bound that. The reference
flags this memory hot spot at modeling_llama.py:696-697),
K11/K12 live in :mod:`relora_amd.ops.optim`,
K13 `merge_and_reinit` in :mod:`relora_amd.relora`, K14 pruning in
:mod:`relora_amd.training_utils`.
"""

import os

import torch
import torch.nn.functional as F

from relora_amd.ops import hip

# ---------------------------------------------------------------------------
# RMSNorm (K5) — reference numerics: fp32 variance, bf16 product
# (reference modeling_llama.py:74-91)
# ---------------------------------------------------------------------------


def rmsnorm_torch(x, weight, eps):
    variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = x * torch.rsqrt(variance + eps)
    if weight.dtype in (torch.float16, torch.bfloat16):
        h = h.to(weight.dtype)
    return weight * h


class _HipRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        x2d = x.contiguous().view(-1, x.shape[-1])
        y, invrms = hip.ext().rmsnorm_fwd(x2d, weight, eps)
        ctx.save_for_backward(x2d, weight, invrms)
        ctx.shape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, invrms = ctx.saved_tensors
        dy2d = dy.contiguous().view(-1, dy.shape[-1])
        dx, dw = hip.ext().rmsnorm_bwd(x2d, weight, invrms, dy2d)
        return dx.view(ctx.shape), dw.to(weight.dtype), None


def rmsnorm(x, weight, eps=1e-6):
    if hip.use_hip(x, "rmsnorm"):
        return _HipRMSNorm.apply(x, weight, eps)
    return rmsnorm_torch(x, weight, eps)


class _HipAddRMSNorm(torch.autograd.Function):
    """Fused `sum = x + residual; normed = rmsnorm(sum)` (K16).  Backward
    returns the SAME gradient tensor for both inputs (d sum/dx = d sum/dres
    = 1) with the residual fork's `+dsum` folded into the dx epilogue — the
    unfused form costs one [M,H] add kernel in each direction.

    Note: because the two returned gradients alias one tensor, calling this
    on two LEAF tensors makes their `.grad`s aliases as well (fine for
    values; an in-place edit of one would show in the other).  The model
    only ever feeds activations, whose gradients are consumed, not stored.
    """

    @staticmethod
    def forward(ctx, x, residual, weight, eps):
        shape = x.shape
        x2d = x.contiguous().view(-1, shape[-1])
        r2d = residual.contiguous().view(-1, shape[-1])
        y, s, invrms = hip.ext().rmsnorm_fwd_add(x2d, r2d, weight, eps)
        ctx.save_for_backward(s, weight, invrms)
        ctx.shape = shape
        return y.view(shape), s.view(shape)

    @staticmethod
    def backward(ctx, dy, dsum):
        s, weight, invrms = ctx.saved_tensors
        H = s.shape[-1]
        dy2d = dy.contiguous().view(-1, H)
        if dsum is None:
            dx, dw = hip.ext().rmsnorm_bwd(s, weight, invrms, dy2d)
        else:
            dx, dw = hip.ext().rmsnorm_bwd_add(s, weight, invrms, dy2d,
                                               dsum.contiguous().view(-1, H))
        dx = dx.view(ctx.shape)
        return dx, dx, dw.to(weight.dtype), None


def add_rmsnorm(x, residual, weight, eps=1e-6):
    """(normed, sum) where sum = x + residual, normed = rmsnorm(sum).
    Same bf16 rounding as the unfused composition."""
    if hip.use_hip(x, "rmsnorm") and x.dtype == torch.bfloat16 \
            and residual.dtype == torch.bfloat16:
        return _HipAddRMSNorm.apply(x, residual, weight, eps)
    s = x + residual
    return rmsnorm(s, weight, eps), s


# ---------------------------------------------------------------------------
# LayerNorm (K6) — pythia path
# ---------------------------------------------------------------------------


class _HipLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x2d = x.contiguous().view(-1, x.shape[-1])
        y, mean, invstd = hip.ext().layernorm_fwd(x2d, weight, bias, eps)
        ctx.save_for_backward(x2d, weight, mean, invstd)
        ctx.shape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, mean, invstd = ctx.saved_tensors
        dy2d = dy.contiguous().view(-1, dy.shape[-1])
        dx, dw, db = hip.ext().layernorm_bwd(x2d, weight, mean, invstd, dy2d)
        return dx.view(ctx.shape), dw.to(weight.dtype), db.to(weight.dtype), None


def layernorm(x, weight, bias, eps=1e-5):
    if hip.use_hip(x, "layernorm"):
        return _HipLayerNorm.apply(x, weight, bias, eps)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


# ---------------------------------------------------------------------------
# RoPE (K4) — rotate_half convention (reference modeling_llama.py:126-141),
# partial-rotary support for pythia (modeling_pythia.py:184-197)
# ---------------------------------------------------------------------------


def rotate_half(x):
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2 :]
    return torch.cat((-x2, x1), dim=-1)


def build_rope_cache(rot_dim, seq_len, base=10000.0, device=None):
    """fp32 cos/sin tables of shape [seq_len, rot_dim] (duplicated halves),
    identical to the reference's `emb = cat((freqs, freqs))` layout."""
    inv_freq = 1.0 / (base ** (torch.arange(0, rot_dim, 2, dtype=torch.float32, device=device) / rot_dim))
    t = torch.arange(seq_len, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


def rope_torch(q, k, cos, sin, position_ids=None):
    """q: [B, nh, S, hd], k: [B, nkv, S, hd] (nkv may be smaller than nh:
    grouped-query attention); cos/sin: [S_cache, rot_dim] fp32.

    Rotates the first rot_dim features, passes the rest through.
    """
    rot = cos.shape[-1]
    S = q.shape[-2]
    if position_ids is None:
        c = cos[:S].to(q.dtype)
        s = sin[:S].to(q.dtype)
    else:
        c = cos[position_ids].to(q.dtype).unsqueeze(1)
        s = sin[position_ids].to(q.dtype).unsqueeze(1)
    q_rot, q_pass = q[..., :rot], q[..., rot:]
    k_rot, k_pass = k[..., :rot], k[..., rot:]
    q_out = (q_rot * c) + (rotate_half(q_rot) * s)
    k_out = (k_rot * c) + (rotate_half(k_rot) * s)
    if q_pass.shape[-1]:
        q_out = torch.cat((q_out, q_pass), dim=-1)
        k_out = torch.cat((k_out, k_pass), dim=-1)
    return q_out, k_out


class _HipRoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin):
        # the kernel reads BHSD-contiguous AND transposed-BSHD views directly
        # (same stride support as attention — no copies on the q/k path);
        # it runs once per tensor, so k may have fewer heads and its own layout
        if not _attn_layout_ok(q):
            q = q.contiguous()
        if not _attn_layout_ok(k):
            k = k.contiguous()
        # Kernel contract: fp32 contiguous tables (a model .to(bf16) casts
        # registered buffers; converting [S,hd] back is noise next to the GEMMs).
        cos = cos.float().contiguous()
        sin = sin.float().contiguous()
        qo, ko = hip.ext().rope_fwd(q, k, cos, sin, False)
        ctx.save_for_backward(cos, sin)
        return qo, ko

    @staticmethod
    def backward(ctx, dqo, dko):
        cos, sin = ctx.saved_tensors
        if not _attn_layout_ok(dqo):
            dqo = dqo.contiguous()
        if not _attn_layout_ok(dko):
            dko = dko.contiguous()
        dq, dk = hip.ext().rope_fwd(dqo, dko, cos, sin, True)
        return dq, dk, None, None


def rope(q, k, cos, sin, position_ids=None):
    """Apply rotary embedding to q and k. position_ids only supported on the
    torch path (training uses the contiguous [0..S) default)."""
    if position_ids is None and hip.use_hip(q, "rope"):
        return _HipRoPE.apply(q, k, cos, sin)
    return rope_torch(q, k, cos, sin, position_ids)


# ---------------------------------------------------------------------------
# Per-head QK RMSNorm + RoPE (Qwen3 convention): RMSNorm over head_dim of
# every head of q and k, one [head_dim] weight per tensor, then the rotary
# embedding.  One HIP kernel in each direction (ops/csrc/qk_norm_rope.hip).
# ---------------------------------------------------------------------------


def qk_norm_rope_torch(q, k, wq, wk, cos, sin, eps, position_ids=None):
    """rmsnorm_torch over the last dim of q and k, then rope_torch."""
    return rope_torch(rmsnorm_torch(q, wq, eps), rmsnorm_torch(k, wk, eps),
                      cos, sin, position_ids)


class _HipQKNormRope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, wq, wk, cos, sin, eps):
        if not _attn_layout_ok(q):
            q = q.contiguous()
        if not _attn_layout_ok(k):
            k = k.contiguous()
        # kernel contract, as for _HipRoPE: fp32 contiguous tables
        cos = cos.float().contiguous()
        sin = sin.float().contiguous()
        wq, wk = wq.contiguous(), wk.contiguous()
        qo, ko, iq, ik = hip.ext().qk_norm_rope_fwd(q, k, wq, wk, cos, sin, eps)
        ctx.save_for_backward(q, k, wq, wk, iq, ik, cos, sin)
        return qo, ko

    @staticmethod
    def backward(ctx, dqo, dko):
        q, k, wq, wk, iq, ik, cos, sin = ctx.saved_tensors
        # the kernel walks dy with x's strides
        if not _same_layout(dqo, q):
            dqo = torch.empty_like(q).copy_(dqo)
        if not _same_layout(dko, k):
            dko = torch.empty_like(k).copy_(dko)
        dq, dk, dwq, dwk = hip.ext().qk_norm_rope_bwd(dqo, dko, q, k, wq, wk, iq, ik, cos, sin)
        return dq, dk, dwq.to(wq.dtype), dwk.to(wk.dtype), None, None, None


def _qk_norm_rope_hip_ok(q, k, wq, wk, cos, sin):
    """What qk_norm_rope_fwd takes: bf16 q, k and weights, head_dim a multiple
    of 16 and <= 128, full rotary, tables that cover the sequence.  head_dim
    52 (llama_40m), fp32 and partial rotary are the torch composition's."""
    hd = q.shape[-1]
    return (q.dim() == 4 and k.dim() == 4
            and q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16
            and wq.dtype == torch.bfloat16 and wk.dtype == torch.bfloat16
            and k.device == q.device
            and k.shape[0] == q.shape[0] and k.shape[2:] == q.shape[2:]
            and hd % 16 == 0 and hd <= 128
            and wq.shape == (hd,) and wk.shape == (hd,)
            and cos.dim() == 2 and cos.shape == sin.shape
            and cos.shape[1] == hd and cos.shape[0] >= q.shape[2]
            and all(t.data_ptr() % 16 == 0 and t.storage_offset() % 8 == 0
                    for t in (q, k, wq, wk)))


def qk_norm_rope(q, k, wq, wk, cos, sin, eps=1e-6, position_ids=None):
    """Per-head RMSNorm of q [B, nh, S, hd] and k [B, nkv, S, hd] with the
    weights wq, wk [hd], then the rotary embedding: the q/k treatment of
    Qwen3-style attention.  position_ids (the kv-cache path) is supported on
    the torch path only, like `rope`."""
    if (position_ids is None and hip.use_hip(q, "qk_norm")
            and _qk_norm_rope_hip_ok(q, k, wq, wk, cos, sin)):
        return _HipQKNormRope.apply(q, k, wq, wk, cos, sin, float(eps))
    return qk_norm_rope_torch(q, k, wq, wk, cos, sin, eps, position_ids)


# ---------------------------------------------------------------------------
# SwiGLU (K7)
# ---------------------------------------------------------------------------


def swiglu_torch(gate, up):
    return F.silu(gate) * up


class _HipSwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        gate = gate.contiguous()
        up = up.contiguous()
        y = hip.ext().swiglu_fwd(gate, up)
        ctx.save_for_backward(gate, up)
        return y

    @staticmethod
    def backward(ctx, dy):
        gate, up = ctx.saved_tensors
        dgate, dup = hip.ext().swiglu_bwd(gate, up, dy.contiguous())
        return dgate, dup


def swiglu(gate, up):
    if hip.use_hip(gate, "swiglu"):
        return _HipSwiGLU.apply(gate, up)
    return swiglu_torch(gate, up)


# ---------------------------------------------------------------------------
# GELU (K8) — pythia MLP, exact erf form (reference modeling_pythia.py:395-406)
# ---------------------------------------------------------------------------


class _HipGELU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return hip.ext().gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return hip.ext().gelu_bwd(x, dy.contiguous())


def gelu(x):
    if hip.use_hip(x, "gelu"):
        return _HipGELU.apply(x)
    return F.gelu(x)


# ---------------------------------------------------------------------------
# Flash attention (K3) — causal, no padding mask (parity with the reference:
# SDPA is_causal=True and padding mask ignored, modeling_llama.py:221-224)
# ---------------------------------------------------------------------------


def doc_starts_from_eos(input_ids, eos_token_id):
    """int32 [B, S]: for every token the index of the first token of its
    document, the `doc_start` of `flash_attention`.  The token after an
    `eos` starts a new document (the `eos` belongs to the document it ends)
    and position 0 always starts one.  Compare / where / cummax only: works
    on CPU and GPU and never synchronises."""
    S = input_ids.shape[-1]
    pos = torch.arange(S, device=input_ids.device).expand_as(input_ids)
    starts = torch.zeros_like(input_ids, dtype=torch.bool)
    starts[..., 1:] = input_ids[..., :-1] == eos_token_id
    starts[..., 0] = True
    marked = torch.where(starts, pos, torch.zeros_like(pos))
    return marked.cummax(dim=-1).values.to(torch.int32)


def doc_mask(doc_start, S):
    """bool [B, 1, S, S], True where query i may attend to kv j:
    doc_start[b, i] <= j <= i."""
    pos = torch.arange(S, device=doc_start.device)
    i, j = pos[:, None], pos[None, :]
    return ((j <= i) & (j >= doc_start[:, :, None].long())).unsqueeze(1)


def sdpa_torch(q, k, v, causal=True, dropout_p=0.0, scale=None, doc_start=None):
    """SDPA with the HIP path's head mapping: with fewer kv heads than query
    heads, query head h reads kv head h // n_rep (HF `repeat_kv`).  The
    expansion is a `repeat_interleave` on the head axis, so autograd sums
    dK/dV back over each group and returns them as [B, nkv, S, hd].

    With `doc_start` (int32 [B, S], see `flash_attention`) the causal mask is
    replaced by the boolean intra-document mask `doc_mask`."""
    nh, nkv = q.shape[1], k.shape[1]
    if nkv != nh:
        if nh % nkv != 0:
            raise ValueError(f"kv heads ({nkv}) must divide query heads ({nh})")
        k = k.repeat_interleave(nh // nkv, dim=1)
        v = v.repeat_interleave(nh // nkv, dim=1)
    if doc_start is not None:
        _check_doc_start(q, k, causal, doc_start)
        return F.scaled_dot_product_attention(
            q, k, v, attn_mask=doc_mask(doc_start, q.shape[-2]), dropout_p=dropout_p,
            scale=scale)
    return F.scaled_dot_product_attention(
        q, k, v, dropout_p=dropout_p, is_causal=causal, scale=scale)


def _check_doc_start(q, k, causal, doc_start):
    if not causal:
        raise ValueError("doc_start requires causal=True")
    if q.shape[-2] != k.shape[-2]:
        raise ValueError(f"doc_start requires equal q and kv lengths, got "
                         f"{q.shape[-2]} and {k.shape[-2]}")
    if tuple(doc_start.shape) != (q.shape[0], q.shape[-2]):
        raise ValueError(f"doc_start must be [B, S] = [{q.shape[0]}, {q.shape[-2]}], "
                         f"got {tuple(doc_start.shape)}")
    if doc_start.dtype != torch.int32:
        raise ValueError(f"doc_start must be int32, got {doc_start.dtype}")


def _attn_layout_ok(t):
    """BHSD-contiguous, or a transposed view of a BSHD buffer (what the
    model's `.view(B,S,nh,hd).transpose(1,2)` produces) — the kernels read
    both directly, so no permute+contiguous copies happen around attention."""
    if t.stride(-1) != 1:
        return False
    B, nh, S, hd = t.shape
    s = tuple(t.stride())
    return (t.is_contiguous()
            or s == (S * nh * hd, hd, nh * hd, 1))


def _same_layout(a, b):
    """equal shapes, and equal strides wherever a stride addresses anything
    (a size-1 dim's stride is arbitrary)"""
    return a.shape == b.shape and all(
        sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


class _HipFlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, doc_start=None):
        # q has its own stride triple, k/v share a second one ([B, nkv, S, hd],
        # nkv dividing nh): copy only the side whose layout the kernels can't read
        if not _attn_layout_ok(q):
            q = q.contiguous()
        if not (_attn_layout_ok(k) and _attn_layout_ok(v) and _same_layout(k, v)):
            k, v = k.contiguous(), v.contiguous()
        if doc_start is None:
            o, lse = hip.ext().attn_fwd(q, k, v, scale)
            ctx.save_for_backward(q, k, v, o, lse)
        else:
            doc_start = doc_start.contiguous()
            o, lse = hip.ext().attn_fwd(q, k, v, scale, doc_start)
            ctx.save_for_backward(q, k, v, o, lse, doc_start)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        # the host copies `do` into q's layout only if it differs
        dq, dk, dv = hip.ext().attn_bwd(q, k, v, o, lse, do, ctx.scale, *doc)
        return dq, dk, dv, None, None


def _attn_hip_supported(q):
    """What the HIP attention kernels take: bf16, head_dim <= 128 and a
    multiple of 8 (every row is read as 16-byte bf16x8 vectors).  Anything
    else is SDPA's, by contract rather than by an error from inside the
    extension.  Of the shipped configs that moves one: llama_40m has
    head_dim 52 (416 / 8), whose rows are only 8-byte aligned; it used to
    run the kernels on misaligned vector loads with no numerics test, and
    now takes SDPA.  Every other config (head_dim 32, 48, 64, 80, 128)
    stays on the HIP path."""
    hd = q.shape[-1]
    return q.dtype == torch.bfloat16 and hd <= 128 and hd % 8 == 0


def _pad32(hd):
    return (hd + 31) // 32 * 32


def flash_attention(q, k, v, causal=True, dropout_p=0.0, scale=None, doc_start=None):
    """q: [B, nh, S, hd]; k, v: [B, nkv, S_kv, hd] with nkv dividing nh
    (grouped-query attention: query head h reads kv head h // (nh // nkv))
    -> [B, nh, S, hd].

    `doc_start` (int32 [B, S] on q's device, the same for all heads) turns on
    intra-document masking for packed rows: doc_start[b, i] is the index of
    the first token of the document token i belongs to, and query i attends
    to kv j iff doc_start[b, i] <= j <= i (`doc_starts_from_eos` builds it).
    It needs causal=True and S == S_kv.  The HIP kernels take it where they
    take the plain call AND the head dim pads to <= 64 (shipped head dims 32,
    48, 64); everything else (80, 128, 52, fp32, CPU) runs SDPA with the
    boolean mask."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if k.shape != v.shape:
        raise ValueError(f"k and v must have one shape, got {tuple(k.shape)} "
                         f"and {tuple(v.shape)}")
    if k.shape[1] < 1 or q.shape[1] % k.shape[1] != 0:
        raise ValueError(f"kv heads ({k.shape[1]}) must divide query heads "
                         f"({q.shape[1]})")
    if doc_start is not None:
        _check_doc_start(q, k, causal, doc_start)
    if (causal and dropout_p == 0.0 and _attn_hip_supported(q)
            and k.dtype == q.dtype and v.dtype == q.dtype
            and hip.use_hip(q, "attention")):
        if doc_start is None:
            return _HipFlashAttention.apply(q, k, v, scale)
        if _pad32(q.shape[-1]) <= 64:
            return _HipFlashAttention.apply(q, k, v, scale, doc_start)
    return sdpa_torch(q, k, v, causal=causal, dropout_p=dropout_p, scale=scale,
                      doc_start=doc_start)


# ---------------------------------------------------------------------------
# Fused chunked cross-entropy over the LM head (K10).
# loss = CE(shift(hidden @ Wᵀ), shift(labels)) without materializing fp32
# logits: per-M-chunk bf16 GEMM + one-pass fp32 row stats (HIP) and an
# in-place softmax-minus-onehot gradient kernel in backward.  Peak logits
# memory is one [chunk, V] bf16 buffer (the full [M, V] only in the default
# single-chunk config, sized for 288 GB HBM — see _CE_CHUNK below).
# ---------------------------------------------------------------------------

# 288 GB HBM comfortably holds one [M,V] bf16 logits buffer for the flagship
# shapes (16384 x 50304 = 1.6 GB), so default to a single chunk: fewer, larger
# GEMMs and no fp32 dw accumulation pass. Shrink via env on smaller cards.
_CE_CHUNK = int(os.environ.get("RELORA_AMD_CE_CHUNK", "16384"))
# RELORA_AMD_CE_SAVE_LOGITS trades HBM for time: keep the bf16 logits from
# forward instead of recomputing the [M,V] GEMM in backward (single-chunk
# mode only; ~1 GB at the flagship shape).  Default ON for 288 GB parts —
# measured +0.4-0.5% e2e on two boxes; =0 to disable on small-HBM cards.
_CE_SAVE_LOGITS = os.environ.get("RELORA_AMD_CE_SAVE_LOGITS", "1") == "1"


def _row_stats_torch(logits, labels, ignore_index):
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    safe = labels.clamp_min(0)
    tgt = lf.gather(1, safe.unsqueeze(1)).squeeze(1)
    return lse, tgt


def _row_stats_ex_torch(logits, labels, ignore_index):
    lse, tgt = _row_stats_torch(logits, labels, ignore_index)
    return lse, tgt, logits.float().sum(dim=-1)


def _check_loss_options(z_loss, label_smoothing):
    if not z_loss >= 0.0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")


class _FusedCrossEntropy(torch.autograd.Function):
    """hidden [M,H], weight [V,H], labels [M] -> mean CE over labels != ignore.

    With z_loss (z) or label_smoothing (eps) non-zero the row objective is
        lse - (1-eps)*x_t - (eps/V)*sum_j x_j + z*lse^2
    and forward returns (loss, ce, zl): the objective plus the detached plain
    cross-entropy mean(lse - x_t) and z*mean(lse^2).  With both at 0 it is the
    plain kernel pair and a single output."""

    @staticmethod
    def forward(ctx, hidden, weight, labels, ignore_index, z_loss=0.0, label_smoothing=0.0):
        M = hidden.shape[0]
        device = hidden.device
        ex = z_loss != 0.0 or label_smoothing != 0.0
        lse_all = torch.empty(M, dtype=torch.float32, device=device)
        loss_sum = torch.zeros((), dtype=torch.float32, device=device)
        if ex:
            V = weight.shape[0]
            ce_sum = torch.zeros_like(loss_sum)
            z_sum = torch.zeros_like(loss_sum)
        valid = labels != ignore_index
        n_valid = int(valid.sum().item())
        use_hip = hip.use_hip(hidden, "ce")
        keep_logits = _CE_SAVE_LOGITS and M <= _CE_CHUNK
        saved_logits = None
        for s in range(0, M, _CE_CHUNK):
            e = min(s + _CE_CHUNK, M)
            logits = hidden[s:e] @ weight.t()
            if keep_logits:
                saved_logits = logits
            lab = labels[s:e]
            if not ex:
                if use_hip:
                    lse, tgt = hip.ext().ce_row_stats(logits, lab, ignore_index)
                else:
                    lse, tgt = _row_stats_torch(logits, lab, ignore_index)
                lse_all[s:e] = lse
                vmask = lab != ignore_index
                loss_sum += torch.where(vmask, lse - tgt, torch.zeros_like(lse)).sum()
                continue
            vmask = lab != ignore_index
            if use_hip:
                lse, tgt, rsum = hip.ext().ce_row_stats_ex(logits, lab.contiguous(), ignore_index)
            else:
                lse, tgt, rsum = _row_stats_ex_torch(logits, lab, ignore_index)
            lse_all[s:e] = lse
            zero = torch.zeros_like(lse)
            ce_c = torch.where(vmask, lse - tgt, zero).sum()
            z_c = torch.where(vmask, lse * lse, zero).sum()
            # eps * (x_t - mean_j x_j): what smoothing adds to lse - x_t
            sm_c = torch.where(vmask, tgt - rsum / V, zero).sum()
            ce_sum += ce_c
            z_sum += z_c
            loss_sum += ce_c + label_smoothing * sm_c + z_loss * z_c
        ctx.save_for_backward(hidden, weight, labels, lse_all,
                              saved_logits if saved_logits is not None
                              else hidden.new_empty(0))
        ctx.ignore_index = ignore_index
        ctx.n_valid = max(n_valid, 1)
        ctx.z_loss = z_loss
        ctx.label_smoothing = label_smoothing
        if not ex:
            return loss_sum / max(n_valid, 1)
        ce = ce_sum / max(n_valid, 1)
        zl = z_sum * (z_loss / max(n_valid, 1))
        ctx.mark_non_differentiable(ce, zl)
        return loss_sum / max(n_valid, 1), ce, zl

    @staticmethod
    def backward(ctx, grad_out, *_parts):
        hidden, weight, labels, lse_all, saved_logits = ctx.saved_tensors
        ignore_index = ctx.ignore_index
        z_loss, eps = ctx.z_loss, ctx.label_smoothing
        ex = z_loss != 0.0 or eps != 0.0
        M, H = hidden.shape
        use_hip = hip.use_hip(hidden, "ce")
        dh = torch.empty_like(hidden)
        single_chunk = M <= _CE_CHUNK
        dw_acc = None if single_chunk else torch.zeros(
            weight.shape, dtype=torch.float32, device=weight.device)
        gscale = (grad_out.float() / ctx.n_valid).item() if grad_out.dim() == 0 else None
        for s in range(0, M, _CE_CHUNK):
            e = min(s + _CE_CHUNK, M)
            if saved_logits.numel() and s == 0 and e == M:
                logits = saved_logits
            else:
                logits = hidden[s:e] @ weight.t()
            lab = labels[s:e]
            lse = lse_all[s:e]
            if use_hip:
                # in-place: logits buffer becomes dlogits (same dtype)
                if ex:
                    hip.ext().ce_grad_ex_(logits, lab.contiguous(), lse, gscale,
                                          z_loss, eps, ignore_index)
                else:
                    hip.ext().ce_grad_(logits, lab, lse, gscale, ignore_index)
                dlogits = logits
            else:
                p = torch.exp(logits.float() - lse.unsqueeze(1))
                vmask = (lab != ignore_index)
                if ex:
                    p = p * (1.0 + 2.0 * z_loss * lse).unsqueeze(1) - eps / logits.shape[1]
                p[~vmask] = 0.0
                safe = lab.clamp_min(0)
                p[vmask, safe[vmask]] -= 1.0 - eps
                dlogits = (p * gscale).to(logits.dtype)
            dh[s:e] = dlogits @ weight
            if single_chunk:
                dw = (dlogits.t() @ hidden[s:e]).to(weight.dtype)
            else:
                dw_acc += (dlogits.t() @ hidden[s:e]).float()
        if not single_chunk:
            dw = dw_acc.to(weight.dtype)
        return dh, dw, None, None, None, None


def fused_cross_entropy(hidden, weight, labels, ignore_index=-100, z_loss=0.0,
                        label_smoothing=0.0, return_parts=False):
    """Mean cross-entropy of `hidden @ weight.T` against `labels`.

    hidden: [M, H] (already shifted/flattened); weight: [V, H]; labels: [M].

    z_loss adds the PaLM auxiliary term `z_loss * mean(lse^2)`;
    label_smoothing is `F.cross_entropy`'s argument of that name.  Both
    default to 0, which is the plain kernel path.  return_parts=True returns
    `(loss, ce, zl)`: the optimised objective plus, detached, the plain
    cross-entropy (what perplexity is computed from) and the z-loss term.
    """
    z_loss, label_smoothing = float(z_loss), float(label_smoothing)
    _check_loss_options(z_loss, label_smoothing)
    if z_loss == 0.0 and label_smoothing == 0.0:
        loss = _FusedCrossEntropy.apply(hidden, weight, labels, ignore_index, 0.0, 0.0)
        if return_parts:
            return loss, loss.detach(), torch.zeros_like(loss)
        return loss
    loss, ce, zl = _FusedCrossEntropy.apply(hidden, weight, labels, ignore_index,
                                            z_loss, label_smoothing)
    return (loss, ce, zl) if return_parts else loss


# ---------------------------------------------------------------------------
# LoRA linear (K1+K2): y = x Wᵀ (+b) + s · dropout(x) Aᵀ Bᵀ
# The production GPU path fuses the rank-r update into the main MFMA GEMM
# (lora_gemm.hip); RELORA_AMD_LORA_PATH=torch forces the hipBLASLt
# composition (also the CPU path).
# ---------------------------------------------------------------------------


_lora_seed_counter = [0]


def get_dropout_rng_state():
    """Philox dropout stream position (for bit-exact checkpoint resume)."""
    return _lora_seed_counter[0]


def set_dropout_rng_state(counter):
    _lora_seed_counter[0] = int(counter)


def _next_dropout_seed():
    _lora_seed_counter[0] += 1
    # mix with the torch seed so runs differ when the user reseeds, while
    # successive calls in one run are distinct and deterministic
    return (torch.initial_seed() & 0x7FFFFFFFFFFF) ^ (_lora_seed_counter[0] * 0x9E3779B97F4A7C15)


# The single-kernel fused GEMM+LoRA (ops/csrc/fused_gemm.hip) replaces
# hipBLASLt+lora_add where the measured A/B favors it: aligned shapes with
# K <= 1024 (profiles/fused_gemm_ab.log — fused wins +8..19% on the
# llama_250m shapes; at K >= 2048 the library's deeper-pipelined GEMM wins
# by 6-36%, so those stay composed).  RELORA_AMD_FUSED_K1=0 disables,
# =all forces it on every aligned shape (for A/B runs).
_FUSED_K1 = os.environ.get("RELORA_AMD_FUSED_K1", "1")


def _use_fused_k1(x2d, weight, lora_A):
    if _FUSED_K1 == "0":
        return False
    M, K = x2d.shape
    N = weight.shape[0]
    r = lora_A.shape[0]
    aligned = (M % 256 == 0 and N % 256 == 0 and K % 64 == 0
               and r % 64 == 0 and r <= 256)
    return aligned and (K <= 1024 or _FUSED_K1 == "all")


class _FusedLoRALinear(torch.autograd.Function):
    """GPU path: the rank-r update accumulates into the main GEMM's output
    via the MFMA lora_add kernels; dropout runs fused with a persisted
    packed philox mask that backward replays exactly.  Saves the three
    [M,N]-sized epilogue round trips per Linear of the composed path."""

    @staticmethod
    def forward(ctx, x, weight, bias, lora_A, lora_B, scale, dropout_p, training):
        in_shape = x.shape
        K = in_shape[-1]
        N = weight.shape[0]
        x2d = x.contiguous().view(-1, K)
        use_dropout = dropout_p > 0 and training
        if use_dropout:
            seed = _next_dropout_seed() & 0x7FFFFFFFFFFFFFFF
            xd, mask = hip.ext().dropout_mask_fwd(x2d, dropout_p, seed)
        else:
            xd, mask = x2d, None
        t_u = xd @ lora_A.t()                       # [M, r]
        del xd  # dA re-applies the mask inline in skinny_grad; no need to
                # persist the dropped-out copy (64 MB per flagship linear)
        bs = lora_B * scale                         # [N, r]
        if _use_fused_k1(x2d, weight, lora_A):
            # single-kernel K1+K2: main MFMA GEMM with the rank-r update as
            # an epilogue on the resident accumulators (no [M,N] RMW pass)
            y = hip.ext().fused_lora_gemm(
                x2d, weight, t_u, lora_B,
                bias if bias is not None else x2d.new_empty(0), scale)
        else:
            y = F.linear(x2d, weight, bias)
            hip.ext().lora_add_nt_(y, t_u, bs)      # y += t_u @ bs^T
        ctx.save_for_backward(x2d, mask if mask is not None else x2d.new_empty(0),
                              t_u, weight, lora_A, bs)
        ctx.scale = scale
        ctx.dropout_p = dropout_p if use_dropout else 0.0
        ctx.has_bias = bias is not None
        return y.view(*in_shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2d, mask, t_u, weight, lora_A, bs = ctx.saved_tensors
        scale, p = ctx.scale, ctx.dropout_p
        N = weight.shape[0]
        dy2d = dy.contiguous().view(-1, N)

        u_s = dy2d @ bs                             # [M, r] = s * dy @ B
        dx = dy2d @ weight                          # [M, K] main path
        hip.ext().lora_add_nn_(dx, u_s, lora_A,
                               mask if p > 0 else mask.new_empty(0, dtype=torch.uint8),
                               1.0 / (1.0 - p) if p > 0 else 1.0)

        # dA = u_s^T @ dropout(x), dB = s * dy^T @ t_u = (t_u^T @ dy)^T * s —
        # via the chunked-M skinny_grad kernel (hipBLASLt launches these
        # 32-WG wide); the dropout mask re-applies inline while staging x,
        # and scale/transpose/cast fold into the combine stage
        empty_mask = mask.new_empty(0, dtype=torch.uint8)
        dA = hip.ext().skinny_grad(u_s, x2d, mask if p > 0 else empty_mask,
                                   1.0 / (1.0 - p) if p > 0 else 1.0,
                                   1.0, False, lora_A.dtype)
        dB = hip.ext().skinny_grad(t_u, dy2d, empty_mask, 1.0, scale, True, bs.dtype)
        dw = dy2d.t() @ x2d if ctx.needs_input_grad[1] else None
        dbias = dy2d.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return (dx.view(dy.shape[:-1] + (weight.shape[1],)), dw, dbias,
                dA, dB, None, None, None)


class _QuantizedLoRALinear(torch.autograd.Function):
    """K15 path: frozen W stays NF4/int8-packed end to end.  Forward runs
    the dequant-fused MFMA GEMM (aligned NF4 shapes) or a transient
    materialize; backward re-dequantizes transiently for dX.  Unlike the
    dense path, NO dense [N,K] W is ever saved for backward — the HBM
    footprint of the frozen weights stays at the packed size (the entire
    point of --quantize; reference runs bnb matmul_4bit, relora.py:314-317).
    """

    @staticmethod
    def forward(ctx, x, bias, lora_A, lora_B, scale, dropout_p, training, qw):
        in_shape = x.shape
        K = in_shape[-1]
        N = qw.out_features
        x2d = x.contiguous().view(-1, K)
        M = x2d.shape[0]
        use_dropout = dropout_p > 0 and training
        if use_dropout:
            seed = _next_dropout_seed() & 0x7FFFFFFFFFFFFFFF
            xd, mask = hip.ext().dropout_mask_fwd(x2d, dropout_p, seed)
        else:
            xd, mask = x2d, None
        t_u = xd @ lora_A.t()
        del xd
        r = lora_A.shape[0]
        empty = x2d.new_empty(0)
        aligned = (M % 256 == 0 and N % 256 == 0 and r % 64 == 0
                   and r <= 256 and _FUSED_K1 != "0")
        fused_nf4 = aligned and qw.mode == "4bit" and K % 64 == 0
        fused_i8 = aligned and qw.mode == "8bit" and K % 256 == 0
        if fused_nf4:
            y = hip.ext().fused_nf4_gemm(
                x2d, qw.qdata, qw.absmax, N, t_u, lora_B,
                bias if bias is not None else empty, scale)
        elif fused_i8:
            y = hip.ext().fused_int8_gemm(
                x2d, qw.qdata, qw.absmax, N, t_u, lora_B,
                bias if bias is not None else empty, scale)
        else:
            w = qw.materialize(torch.bfloat16)  # transient; freed below
            y = F.linear(x2d, w, bias)
            del w
            hip.ext().lora_add_nt_(y, t_u, lora_B * scale)
        ctx.save_for_backward(x2d, mask if mask is not None else empty,
                              t_u, lora_A, lora_B)
        ctx.qw = qw
        ctx.scale = scale
        ctx.dropout_p = dropout_p if use_dropout else 0.0
        ctx.has_bias = bias is not None
        return y.view(*in_shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2d, mask, t_u, lora_A, lora_B = ctx.saved_tensors
        scale, p = ctx.scale, ctx.dropout_p
        qw = ctx.qw
        N = qw.out_features
        dy2d = dy.contiguous().view(-1, N)
        bs = lora_B * scale
        u_s = dy2d @ bs
        w = qw.materialize(torch.bfloat16)  # transient dense W for dX only
        dx = dy2d @ w
        del w
        hip.ext().lora_add_nn_(dx, u_s, lora_A,
                               mask if p > 0 else mask.new_empty(0, dtype=torch.uint8),
                               1.0 / (1.0 - p) if p > 0 else 1.0)
        empty_mask = mask.new_empty(0, dtype=torch.uint8)
        dA = hip.ext().skinny_grad(u_s, x2d, mask if p > 0 else empty_mask,
                                   1.0 / (1.0 - p) if p > 0 else 1.0,
                                   1.0, False, lora_A.dtype)
        dB = hip.ext().skinny_grad(t_u, dy2d, empty_mask, 1.0, scale, True, lora_B.dtype)
        dbias = dy2d.sum(0) if ctx.has_bias else None
        return (dx.view(dy.shape[:-1] + (qw.in_features,)), dbias,
                dA, dB, None, None, None, None)


class _HipDropout(torch.autograd.Function):
    """Standalone dropout with the philox packed-bit mask kernels (1 bit per
    element vs torch's byte mask; the composed-path replacement for
    F.dropout on odd-dim linears)."""

    @staticmethod
    def forward(ctx, x, p):
        xc = x.contiguous()
        shape = xc.shape
        seed = _next_dropout_seed() & 0x7FFFFFFFFFFFFFFF
        xd, mask = hip.ext().dropout_mask_fwd(xc.view(-1, shape[-1]), p, seed)
        ctx.save_for_backward(mask)
        ctx.p = p
        return xd.view(shape)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dx = hip.ext().dropout_mask_bwd(dy.contiguous(), mask, ctx.p)
        return dx.view(dy.shape), None


def _fused_ok(x, weight, lora_A, scale, lora_only):
    if weight is None:
        return False
    r = lora_A.shape[0]
    # odd in/out dims (llama_1b intermediate 5461) are CORRECT through the
    # fused kernels (alignment-guarded fallbacks) but measured slower e2e
    # than the composed path even after its scale-folding trim (58.7k vs
    # 66.0k tok/s on the flagship, gpurun r2c A/B) — unaligned rows defeat
    # every vectorized RMW path.  RELORA_AMD_LORA_ODD=fused re-routes them
    # for future A/Bs.
    dims_ok = (x.shape[-1] % 8 == 0 and weight.shape[0] % 8 == 0
               or os.environ.get("RELORA_AMD_LORA_ODD", "torch") == "fused")
    return (hip.use_hip(x, "lora") and not lora_only and not torch.is_tensor(scale)
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and r % 32 == 0 and r <= 256 and dims_ok
            and os.environ.get("RELORA_AMD_LORA_PATH", "fused") != "torch")


def lora_linear(x, weight, bias, lora_A, lora_B, scale, dropout_p=0.0,
                training=False, lora_only=False, quantized_weight=None):
    """y = x W^T (+b) + s * dropout(x) A^T B^T.

    GPU bf16 path: _FusedLoRALinear (MFMA rank-r accumulate kernels).
    Otherwise: composed torch ops (CPU path and the numerics oracle).
    `scale` may be a python float or a 0-d tensor (trainable scaling,
    already passed through tanh by the caller) — tensor scale uses the
    composed path so autograd reaches it.
    """
    if quantized_weight is not None:
        if (hip.use_hip(x, "lora") and not lora_only and not torch.is_tensor(scale)
                and x.dtype == torch.bfloat16):
            return _QuantizedLoRALinear.apply(x, bias, lora_A, lora_B,
                                              float(scale), dropout_p, training,
                                              quantized_weight)
        # CPU / tensor-scale fallback: transient materialize + composed ops
        weight = quantized_weight.materialize(x.dtype if x.is_floating_point()
                                              else torch.float32)
    if _fused_ok(x, weight, lora_A, scale, lora_only):
        return _FusedLoRALinear.apply(x, weight, bias, lora_A, lora_B,
                                      float(scale), dropout_p, training)
    if dropout_p > 0 and training and x.is_cuda and x.dtype == torch.bfloat16 \
            and hip.use_hip(x, "dropout"):
        xd = _HipDropout.apply(x, dropout_p)  # packed 1-bit mask, philox
    elif dropout_p > 0:
        xd = F.dropout(x, p=dropout_p, training=training)
    else:
        xd = x
    if x.is_cuda:
        # fold the scale into the [M,r] intermediate (45x smaller than the
        # [M,N] product the naive composition scales) — same math, removes
        # a full-size elementwise pass; tensor scale keeps autograd
        lora_out = F.linear(F.linear(xd, lora_A) * scale, lora_B)
        if lora_only:
            return lora_out
        return F.linear(x, weight, bias).add_(lora_out)
    # CPU path stays the bit-exact reference composition (parity oracle)
    lora_out = F.linear(F.linear(xd, lora_A), lora_B)
    if lora_only:
        return lora_out * scale
    return F.linear(x, weight, bias) + lora_out * scale


# ---------------------------------------------------------------------------
# Group LoRA linear: G <= 3 sibling projections that share one input
# (q/k/v, gate/up).  One lora_down_dropout launch reads x once for every
# sibling's dropout + rank-r down-projection, and backward accumulates all
# siblings' input gradients into one dx buffer (ops/csrc/lora_group.cpp).
# RELORA_AMD_LORA_GROUP=0 disables grouping (read at import, for A/B runs).
# ---------------------------------------------------------------------------

_LORA_GROUP = os.environ.get("RELORA_AMD_LORA_GROUP", "1") != "0"
# RELORA_AMD_LORA_GROUP_BWD=0: the group backward calls lora_add_nn_ and
# skinny_grad once per sibling instead of the two group kernels (dx in one
# pass, every dA from one read of x).
_LORA_GROUP_BWD = os.environ.get("RELORA_AMD_LORA_GROUP_BWD", "1") != "0"
# RELORA_AMD_LORA_GROUP_ROPE=0: q and k leave the group op unrotated and
# ops.rope runs on them afterwards (one lora_add_nt_ per sibling, then the
# rope kernel) instead of the rotation in the group's LoRA epilogue.
_LORA_GROUP_ROPE = os.environ.get("RELORA_AMD_LORA_GROUP_ROPE", "1") != "0"


class _LoRALinearGroup(torch.autograd.Function):
    """`tensors` is (weight, bias-or-None, lora_A, lora_B) per sibling,
    flattened; returns one output per sibling.

    `rope` is None or (cos, sin, flags, head_dim), fp32 contiguous tables:
    the outputs of the flagged siblings come back RoPE-rotated (position =
    index along x's second-to-last dim), the rotation done by the LoRA
    epilogue kernel.  Callers check `lora_group_rope_ok` first."""

    @staticmethod
    def forward(ctx, x, scales, dropout_p, training, rope, *tensors):
        G = len(scales)
        Ws, biases = tensors[0::4], tensors[1::4]
        As, Bs = tensors[2::4], tensors[3::4]
        in_shape = x.shape
        K = in_shape[-1]
        x2d = x.contiguous().view(-1, K)
        use_dropout = dropout_p > 0 and training
        # one seed per sibling, in sibling order: the philox stream position
        # and every mask equal what sequential per-module calls produce
        seeds = ([_next_dropout_seed() & 0x7FFFFFFFFFFFFFFF for _ in range(G)]
                 if use_dropout else [])
        empty = x2d.new_empty(0)
        fused = [int(_use_fused_k1(x2d, W, A)) for W, A in zip(Ws, As)]
        rope_args, tables = (), ()
        if rope is not None:
            cos, sin, flags, head_dim = rope
            tables = (cos, sin)
            rope_args = (cos, sin, [int(bool(f)) for f in flags], in_shape[-2], head_dim)
        out = hip.ext().lora_group_fwd(
            x2d, list(Ws), [b if b is not None else empty for b in biases],
            [A.contiguous() for A in As], [B.contiguous() for B in Bs],
            [float(s) for s in scales],
            seeds, dropout_p if use_dropout else 0.0, fused, *rope_args)
        ys, ts, bss = out[:G], out[G:2 * G], out[2 * G:3 * G]
        masks = out[3 * G:]
        ctx.save_for_backward(x2d, *ts, *bss, *masks, *Ws, *As, *tables)
        ctx.rope = None if rope is None else (rope_args[2], rope_args[3], rope_args[4])
        ctx.G = G
        ctx.scales = [float(s) for s in scales]
        ctx.dropout_p = dropout_p if use_dropout else 0.0
        ctx.has_bias = [b is not None for b in biases]
        return tuple(y.view(*in_shape[:-1], y.shape[-1]) for y in ys)

    @staticmethod
    def backward(ctx, *dys):
        G, p = ctx.G, ctx.dropout_p
        saved = ctx.saved_tensors
        x2d = saved[0]
        ts, bss = saved[1:1 + G], saved[1 + G:1 + 2 * G]
        nm = G if p > 0 else 0
        masks = saved[1 + 2 * G:1 + 2 * G + nm]
        Ws = saved[1 + 2 * G + nm:1 + 3 * G + nm]
        As = saved[1 + 3 * G + nm:1 + 4 * G + nm]
        dy2d = [dy.contiguous().view(-1, W.shape[0]) for dy, W in zip(dys, Ws)]
        if ctx.rope is not None:
            # undo the rotation on the gradients of the rotated outputs, out
            # of place (an incoming gradient may be shared), q and k in one
            # launch; from here on backward is that of the unrotated op
            cos, sin = saved[1 + 4 * G + nm:3 + 4 * G + nm]
            flags, S, hd = ctx.rope
            rot = [g for g in range(G) if flags[g]]
            for i in range(0, len(rot), 2):
                pair = [dy2d[g].view(-1, S, dy2d[g].shape[1] // hd, hd).transpose(1, 2)
                        for g in rot[i:i + 2]]
                if len(pair) == 1:  # no partner: a tensor without heads
                    pair.append(pair[0].new_empty(pair[0].shape[0], 0, S, hd))
                res = hip.ext().rope_fwd(pair[0], pair[1], cos, sin, True)
                for g, d in zip(rot[i:i + 2], res):
                    dy2d[g] = d.transpose(1, 2).reshape(-1, dy2d[g].shape[1])
        out = hip.ext().lora_group_bwd(
            dy2d, x2d, list(masks), list(ts), list(Ws),
            [A.contiguous() for A in As], list(bss), ctx.scales, p,
            _LORA_GROUP_BWD)
        dx, dAs, dBs = out[0], out[1:1 + G], out[1 + G:1 + 2 * G]
        grads = []
        for g in range(G):
            # needs_input_grad index: 5 leading non-sibling args, 4 per sibling
            dw = dy2d[g].t() @ x2d if ctx.needs_input_grad[5 + 4 * g] else None
            dbias = (dy2d[g].sum(0)
                     if ctx.has_bias[g] and ctx.needs_input_grad[6 + 4 * g] else None)
            grads += [dw, dbias, dAs[g], dBs[g]]
        return (dx.view(dys[0].shape[:-1] + (x2d.shape[1],)), None, None, None, None,
                *grads)


def lora_group_ok(x, specs):
    """Shapes and dtypes the group op takes: bf16 on the HIP path, K % 8 == 0,
    one shared r with r % 32 == 0 and r <= 128, float scales, 1..3 siblings.
    The kernels take r <= 256, but at r = 256 lora_down_dropout measured
    slower than the launches it replaces (174 vs 101 us at G=2, 247 vs 152 us
    at G=3) and llama_7b did not gain, so r > 128 keeps the per-linear path
    (profiles/stage6_lora_group.md)."""
    if not (_LORA_GROUP and 1 <= len(specs) <= 3):
        return False
    if x.dtype != torch.bfloat16 or not hip.use_hip(x, "lora"):
        return False
    if os.environ.get("RELORA_AMD_LORA_PATH", "fused") == "torch":
        return False
    K = x.shape[-1]
    r = specs[0][2].shape[0]
    if K % 8 != 0 or r % 32 != 0 or r > 128:
        return False
    for weight, bias, lora_A, lora_B, scale in specs:
        if weight is None or torch.is_tensor(scale):
            return False
        if weight.dtype != torch.bfloat16 or lora_A.dtype != torch.bfloat16:
            return False
        if lora_A.shape != (r, K) or weight.shape[1] != K:
            return False
    return True


def lora_group_rope_ok(x, specs, rope):
    """Whether the group op can rotate the flagged outputs in its LoRA
    epilogue (lora_add_nt_rope_group_), given that `lora_group_ok(x, specs)`
    holds.  `rope` is (cos, sin, flags, head_dim).  The kernel takes full
    rotary over heads of 64 or 128 columns, N % 128 == 0 for every sibling,
    x of shape [..., S, K] with S inside the tables, and fp32 contiguous
    tables; a group with a sibling that the single-linear rule routes to
    fused_lora_gemm (K <= 1024) keeps the separate rope pass, as does
    RELORA_AMD_LORA_GROUP_ROPE=0."""
    cos, sin, flags, hd = rope
    if not (_LORA_GROUP_ROPE and x.dim() >= 2 and len(flags) == len(specs) and any(flags)):
        return False
    if hd not in (64, 128) or cos.dim() != 2 or cos.shape != sin.shape:
        return False
    if cos.shape[1] != hd or cos.shape[0] < x.shape[-2]:
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               and t.data_ptr() % 16 == 0 for t in (cos, sin)):
        return False
    x2d = x.view(-1, x.shape[-1]) if x.is_contiguous() else x.reshape(-1, x.shape[-1])
    for weight, _, lora_A, _, _ in specs:
        if weight.shape[0] % 128 != 0 or weight.shape[0] % hd != 0:
            return False
        if _use_fused_k1(x2d, weight, lora_A):
            return False
    return True


def lora_linear_group(x, specs, dropout_p=0.0, training=False, rope=None):
    """[lora_linear(x, *spec) for spec in specs] for siblings that share the
    input `x`, as one group op.  `specs` is a list of (weight, bias, lora_A,
    lora_B, scale); callers check `lora_group_ok` first.  With `rope` =
    (cos, sin, flags, head_dim) the flagged outputs come back rotated;
    callers check `lora_group_rope_ok` too."""
    flat = []
    for weight, bias, lora_A, lora_B, _ in specs:
        flat += [weight, bias, lora_A, lora_B]
    if rope is not None:
        rope = (rope[0], rope[1], tuple(bool(f) for f in rope[2]), int(rope[3]))
    return list(_LoRALinearGroup.apply(
        x, tuple(float(s[4]) for s in specs), dropout_p, training, rope, *flat))
