"""Frozen-weight quantization (K15): blockwise NF4 and int8, row-wise fp8, MXFP4.

MI355X-native replacement for the reference's bitsandbytes usage
(reference relora.py:225-238, 277-299): the frozen `W` of a wrapped Linear
lives quantized at rest (4-bit NF4 with fp32 absmax per 64-element block,
or symmetric linear int8 per 256-element block) and is dequantized into a
transient bf16 buffer for each GEMM; the ReLoRA merge runs
dequant -> W += s·BA -> requant (the reference's exact flow).

`fp8` stores OCP e4m3 codes with one fp32 absmax per output row; on aligned
shapes its forward GEMM runs on the codes themselves (f8f6f4 matrix
instructions, relora_amd/ops/csrc/fp8_gemm.hip) with the activations
quantised per token row.

`mxfp4` stores OCP MX blocks along K: e2m1 codes, two a byte, and one E8M0
scale byte per 32 elements (4.25 bits per weight).  On aligned shapes the
forward multiplies the e4m3 activations of the fp8 mode with the codes as
stored, on the block-scaled matrix instructions
(relora_amd/ops/csrc/mxfp4_gemm.hip).

GPU path: relora_amd/ops/csrc/quantize.hip.  The pure-python reference
implementations here are the CPU path and the kernels' numerics oracle.
"""

import torch
import torch.nn as nn

from relora_amd.ops import hip

NF4_CODE = torch.tensor([
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
    -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
    0.07958029955625534, 0.16093020141124725, 0.24611230194568634,
    0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
    0.7229568362236023, 1.0], dtype=torch.float32)

NF4_BLOCK = 64
I8_BLOCK = 256


def quantize_nf4_ref(x):
    """python oracle: x (any shape, even numel) -> (packed uint8, absmax)."""
    flat = x.detach().float().reshape(-1)
    n = flat.numel()
    nblocks = (n + NF4_BLOCK - 1) // NF4_BLOCK
    padded = torch.zeros(nblocks * NF4_BLOCK, dtype=torch.float32)
    padded[:n] = flat
    blocks = padded.view(nblocks, NF4_BLOCK)
    absmax = blocks.abs().amax(dim=1)
    scaled = blocks / absmax.clamp_min(1e-30).unsqueeze(1)
    scaled[absmax == 0] = 0.0
    idx = (scaled.unsqueeze(-1) - NF4_CODE).abs().argmin(dim=-1).to(torch.uint8)
    idx = idx.view(-1)[:n].view(n // 2, 2)
    packed = (idx[:, 0] << 4) | idx[:, 1]
    return packed.contiguous(), absmax


def dequantize_nf4_ref(packed, absmax, n, dtype=torch.float32):
    hi = (packed >> 4).long()
    lo = (packed & 0xF).long()
    out = torch.empty(n, dtype=torch.float32)
    out[0::2] = NF4_CODE[hi]
    out[1::2] = NF4_CODE[lo]
    blocks = torch.arange(n) // NF4_BLOCK
    out = out * absmax[blocks]
    return out.to(dtype)


def quantize_int8_ref(x):
    flat = x.detach().float().reshape(-1)
    n = flat.numel()
    nblocks = (n + I8_BLOCK - 1) // I8_BLOCK
    padded = torch.zeros(nblocks * I8_BLOCK, dtype=torch.float32)
    padded[:n] = flat
    blocks = padded.view(nblocks, I8_BLOCK)
    absmax = blocks.abs().amax(dim=1)
    scale = torch.where(absmax > 0, 127.0 / absmax, torch.zeros_like(absmax))
    q = torch.round(blocks * scale.unsqueeze(1)).clamp(-127, 127).to(torch.int8)
    return q.view(-1)[:n].contiguous(), absmax


def dequantize_int8_ref(q, absmax, n, dtype=torch.float32):
    blocks = torch.arange(n) // I8_BLOCK
    out = q.float() * (absmax[blocks] / 127.0)
    return out.to(dtype)


FP8_MAX = 448.0  # largest finite e4m3fn value


def quantize_fp8_ref(x, col_scale=None):
    """python oracle: x [R, K] -> (e4m3 codes uint8 [R, K], absmax fp32 [R]).

    Per row: inv = 448/absmax (one fp32 division), code = e4m3_rne(v*inv)
    with the product in fp32; a row of zeros gives zero codes.

    `col_scale` (fp32 [K], the absmax of a row-quantised W whose rows are
    x's columns): the rule applies to g = x * (col_scale/448) instead, the
    quotient one fp32 division and the product rounded once to fp32 (the
    oracle of `quantize_rows_fp8_scaled`, the fp8 backward's quantiser)."""
    v = x.detach().float()
    if col_scale is not None:
        cs = col_scale.detach().float()
        if cs.shape != (v.shape[1],):
            raise ValueError(f"col_scale must have shape ({v.shape[1]},), got {tuple(cs.shape)}")
        v = v * (cs / torch.full_like(cs, FP8_MAX)).unsqueeze(0)
    absmax = v.abs().amax(dim=1)
    # a tensor numerator: `448.0 / absmax` would be reciprocal-then-multiply,
    # two roundings where the format asks for one division
    inv = torch.where(absmax > 0, torch.full_like(absmax, FP8_MAX) / absmax,
                      torch.zeros_like(absmax))
    codes = (v * inv.unsqueeze(1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.contiguous(), absmax


def dequantize_fp8_ref(codes, absmax, dtype=torch.float32):
    """value = float(code) * (absmax/448) in fp32, rounded once to `dtype`."""
    v = codes.view(torch.float8_e4m3fn).float() * (absmax.float() / FP8_MAX).unsqueeze(1)
    return v.to(dtype)


MX_BLOCK = 32
E2M1_VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def quantize_mxfp4_ref(w):
    """python oracle and definition of the format: w [N, K] ->
    (codes uint8 [N, Kp/2], scales uint8 [N, Kp/32]), Kp = K rounded up to 32.

    A block is 32 consecutive k of one row; a short last block is padded with
    zeros, which encode as zero codes.  Scale byte (E8M0, value 2^(byte-127)):
    clamp(E - 2, 0, 254) with E the biased exponent field of the block's fp32
    amax, 127 for an all-zero block.  Code: e2m1 of v * 2^(127-byte) (exact in
    fp32), magnitude rounded to nearest with ties to the even code and
    saturating at 6, sign in bit 3.  The sign bit of v is always kept, so -0
    and values that round to zero encode as code 8 (they decode to -0).
    Packing: the low nibble of a byte is the lower k."""
    v = w.detach().float()
    N, K = v.shape
    nb = (K + MX_BLOCK - 1) // MX_BLOCK
    padded = torch.zeros(N, nb * MX_BLOCK, dtype=torch.float32)
    padded[:, :K] = v
    blocks = padded.view(N, nb, MX_BLOCK)
    amax = blocks.abs().amax(dim=2)
    e = (amax.view(torch.int32) >> 23) & 0xFF
    byte = torch.where(amax > 0, (e - 2).clamp(0, 254), torch.full_like(e, 127))
    inv = ((254 - byte) << 23).view(torch.float32)      # 2^(127-byte), a normal fp32
    s = blocks * inv.unsqueeze(2)
    a = s.abs()
    mag = ((a > 0.25).int() + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5)
           + (a >= 3.5) + (a > 5.0))
    code = (mag | ((s.view(torch.int32) >> 28) & 8)).view(N, nb * MX_BLOCK // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return codes.contiguous(), byte.to(torch.uint8)


def dequantize_mxfp4_ref(codes, scales, K, dtype=torch.float32):
    """value = e2m1(code) * 2^(byte-127), exact in fp32 and bf16; the padding
    of a short last block is cut off."""
    N = codes.shape[0]
    c = torch.stack((codes & 0xF, codes >> 4), dim=2).view(N, -1).long()
    mag = E2M1_VALUES[c & 7]
    val = torch.where((c & 8) != 0, -mag, mag)
    b = scales.to(torch.int32)
    sc = torch.where(b > 0, b << 23, torch.full_like(b, 0x00400000)).view(torch.float32)
    out = val.view(N, -1, MX_BLOCK) * sc.unsqueeze(2)
    return out.view(N, -1)[:, :K].to(dtype)


def transcode_mxfp4_e4m3_ref(codes, scales, K):
    """python oracle and definition of the MXFP4 backward's B operand:
    (codes [N, K/2], scales [N, K/32]) -> (B uint8 [N, K], E uint8 [K/32]).

    A stripe is one MX block column: the 32 columns k = 32kb .. 32kb+31 over
    all N rows.  E[kb] = max_n scales[n, kb], and
        B[n, k] = e4m3_rne(e2m1(code[n, k]) * 2^(scales[n, kb] - E[kb] + 6)),
    so that W[n, k] = e4m3(B[n, k]) * 2^(E[kb] - 133) wherever B is exact.
    The stripe's largest block lands on 6 * 2^6 = 384 <= 448: no NaN code
    arises.  Every e2m1 magnitude is a multiple of 0.5 and e4m3's subnormal
    step is 2^-9, so B is exact while E - s <= 14; at 15 .. 18 the smallest
    magnitudes round (ties to even) and from 19 on every code is a zero.  The
    sign bit is kept throughout (-0 stays -0).  K % 32 == 0."""
    N = codes.shape[0]
    if K % MX_BLOCK or codes.shape != (N, K // 2) or scales.shape != (N, K // MX_BLOCK):
        raise ValueError(f"need K % 32 == 0, codes [N, K/2] and scales [N, K/32]; got K={K}, "
                         f"{tuple(codes.shape)} and {tuple(scales.shape)}")
    c = torch.stack((codes & 0xF, codes >> 4), dim=2).view(N, K).long()
    mag = E2M1_VALUES.to(codes.device)[c & 7]
    val = torch.where((c & 8) != 0, -mag, mag)
    emax = scales.amax(dim=0)
    # 2^(s - E + 6): the exponent field 133 - (E - s); past a spread of 32
    # everything is flushed anyway, and the field stays that of a normal fp32
    spread = (emax.to(torch.int32).unsqueeze(0) - scales.to(torch.int32)).clamp(max=32)
    factor = ((133 - spread) << 23).view(torch.float32)
    b = (val.view(N, -1, MX_BLOCK) * factor.unsqueeze(2)).to(torch.float8_e4m3fn)
    return b.view(torch.uint8).view(N, K).contiguous(), emax.contiguous()


class QuantizedWeight(nn.Module):
    """A frozen 2-D weight stored quantized (blockwise NF4/int8, row-wise fp8,
    MXFP4 blocks along K).

    Quantization happens on first materialization on a CUDA device (CPU
    keeps the python reference path for tests).  `materialize()` returns a
    dense tensor of the original dtype/shape; `requantize_(w)` re-encodes
    after a ReLoRA merge.
    """

    def __init__(self, weight, mode):
        super().__init__()
        if mode not in ("4bit", "8bit", "fp8", "mxfp4"):
            raise ValueError(f"unknown quantize mode {mode!r}")
        self.mode = mode
        self.out_features, self.in_features = weight.shape
        self.numel = weight.numel()
        self.dtype = weight.dtype
        self._encode(weight.detach())

    def stripe_emax(self):
        """mxfp4: E uint8 [K/32], the largest scale byte of every block column
        (transcode_mxfp4_e4m3_ref).  Cached as a plain attribute, so it is no
        state_dict key; a re-encode drops it, and a device move or an in-place
        load of the scales (load_state_dict) recomputes it."""
        key = (self.absmax.data_ptr(), self.absmax._version)
        if self._emax is None or self._emax[0] != key:
            self._emax = (key, self.absmax.amax(dim=0).contiguous())
        return self._emax[1]

    def _encode(self, w):
        self._emax = None
        if self.mode == "fp8":
            # qdata uint8 [N*K], absmax fp32 [N]: same buffer names as the
            # blockwise modes, so casts and checkpoints treat them alike
            if w.is_cuda:
                q, absmax = hip.ext().quantize_rows_fp8(w.contiguous().to(torch.bfloat16))
            else:
                q, absmax = quantize_fp8_ref(w)
            q = q.view(-1)
        elif self.mode == "mxfp4":
            # qdata: codes uint8 [N, Kp/2]; absmax: the uint8 E8M0 block
            # scales [N, Kp/32] under the buffer name of the other modes
            if w.is_cuda:
                q, absmax = hip.ext().quantize_rows_mxfp4(w.contiguous().to(torch.bfloat16))
            else:
                q, absmax = quantize_mxfp4_ref(w)
        elif w.is_cuda:
            wc = w.contiguous().to(torch.bfloat16)
            if self.mode == "4bit":
                q, absmax = hip.ext().quantize_nf4(wc.view(-1))
            else:
                q, absmax = hip.ext().quantize_int8(wc.view(-1))
        else:
            if self.mode == "4bit":
                q, absmax = quantize_nf4_ref(w)
            else:
                q, absmax = quantize_int8_ref(w)
        self.register_buffer("qdata", q)
        self.register_buffer("absmax", absmax)

    def materialize(self, dtype=None):
        dtype = dtype or self.dtype
        if self.mode == "fp8":
            N, K = self.out_features, self.in_features
            if self.qdata.is_cuda:
                tdtype = torch.bfloat16 if dtype in (torch.bfloat16, torch.float16) else torch.float32
                flat = hip.ext().dequantize_rows_fp8(self.qdata, self.absmax, N, K, tdtype)
            else:
                flat = dequantize_fp8_ref(self.qdata.view(N, K), self.absmax, dtype)
        elif self.mode == "mxfp4":
            N, K = self.out_features, self.in_features
            if self.qdata.is_cuda:
                tdtype = torch.bfloat16 if dtype in (torch.bfloat16, torch.float16) else torch.float32
                flat = hip.ext().dequantize_rows_mxfp4(self.qdata, self.absmax, N, K, tdtype)
            else:
                flat = dequantize_mxfp4_ref(self.qdata, self.absmax, K, dtype)
        elif self.qdata.is_cuda:
            tdtype = torch.bfloat16 if dtype in (torch.bfloat16, torch.float16) else torch.float32
            if self.mode == "4bit":
                flat = hip.ext().dequantize_nf4(self.qdata, self.absmax, self.numel, tdtype)
            else:
                flat = hip.ext().dequantize_int8(self.qdata, self.absmax, self.numel, tdtype)
        else:
            if self.mode == "4bit":
                flat = dequantize_nf4_ref(self.qdata, self.absmax, self.numel, dtype)
            else:
                flat = dequantize_int8_ref(self.qdata, self.absmax, self.numel, dtype)
        return flat.view(self.out_features, self.in_features).to(dtype)

    @torch.no_grad()
    def requantize_(self, w):
        device = self.qdata.device
        self._encode(w.to(device))

    def extra_repr(self):
        return (f"out_features={self.out_features}, in_features={self.in_features}, "
                f"mode={self.mode}")


# absmax must survive model-wide dtype casts (a .to(bf16) on the model would
# otherwise downcast the fp32 scales); mxfp4's are uint8 bytes and stay so
def _quantized_apply(self, fn, recurse=True):
    before = self.absmax
    out = nn.Module._apply(self, fn, recurse)
    if self.mode != "mxfp4" and self.absmax.dtype != torch.float32:
        if self.mode == "fp8":
            # a row scale rounded to bf16 would move the whole row: put the
            # fp32 values back instead of widening the rounded ones
            self.absmax = before.to(self.absmax.device)
        else:
            self.absmax = self.absmax.float()
    return out


QuantizedWeight._apply = _quantized_apply
