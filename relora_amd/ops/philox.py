"""Philox4x32-10 and stochastic fp32 -> bf16 rounding, in numpy integer ops.

This is the reference for the random bits the `fused_adamw_ex` /
`stochastic_round_bf16` HIP kernels draw, and the implementation the CPU
optimizer path uses. It is written from the published algorithm (Salmon et
al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11): ten rounds of

    (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),
                         hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0))

with the key advanced by the Weyl constants between rounds.

Counter layout used by the optimizer (everything survives a checkpoint, no
generator state is consumed):

    key     = (seed low 32, seed high 32)
    counter = (element index low 32, element index high 32, step, ordinal)

One call per element; 16 bits per destination ("lane"):

    lane 0  parameter    low  16 bits of word 0
    lane 1  exp_avg      high 16 bits of word 0
    lane 2  exp_avg_sq   low  16 bits of word 1
"""

import numpy as np
import torch

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85

LANE_PARAM, LANE_EXP_AVG, LANE_EXP_AVG_SQ = 0, 1, 2

_MASK32 = np.uint64(0xFFFFFFFF)
_SHIFT32 = np.uint64(32)


def philox4x32_10(key, counter):
    """Ten-round Philox4x32. `key` is (k0, k1), `counter` is (c0, c1, c2, c3);
    every entry is an int or an integer array (broadcast together). Returns
    four uint32 arrays."""
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    c = [np.asarray(x).astype(np.uint64) & _MASK32 for x in counter]
    shape = np.broadcast_shapes(*(x.shape for x in c))
    c0, c1, c2, c3 = (np.broadcast_to(x, shape) for x in c)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for rnd in range(10):
        if rnd > 0:
            k0 = (k0 + np.uint64(PHILOX_W0)) & _MASK32
            k1 = (k1 + np.uint64(PHILOX_W1)) & _MASK32
        p0 = m0 * c0  # 32x32 -> 64-bit products, exact in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (
            (p1 >> _SHIFT32) ^ c1 ^ k0,
            p1 & _MASK32,
            (p0 >> _SHIFT32) ^ c3 ^ k1,
            p0 & _MASK32,
        )
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def element_words(seed, step, ordinal, index):
    """The four Philox words of elements `index` (int array) of tensor
    `ordinal` at optimizer step `step`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = np.asarray(index).astype(np.uint64)
    return philox4x32_10(
        (seed & 0xFFFFFFFF, seed >> 32),
        (index & _MASK32, index >> _SHIFT32, int(step) & 0xFFFFFFFF, int(ordinal) & 0xFFFFFFFF),
    )


def lane_bits(words, lane):
    """16 random bits per element for destination `lane` (uint32 array)."""
    w0, w1 = words[0], words[1]
    if lane == LANE_PARAM:
        return w0 & np.uint32(0xFFFF)
    if lane == LANE_EXP_AVG:
        return w0 >> np.uint32(16)
    if lane == LANE_EXP_AVG_SQ:
        return w1 & np.uint32(0xFFFF)
    raise ValueError(f"lane must be 0, 1 or 2, got {lane}")


def round_bits_to_bf16(u, r16):
    """The rounding rule on raw bit patterns: `u` uint32 fp32 patterns, `r16`
    16 random bits each. Returns the uint16 bf16 patterns.

    Finite values: upper 16 bits of `u + r16` — the magnitude rounds up with
    probability low16(u)/65536, exact values never move, and a carry out of
    the largest finite exponent gives inf. inf/nan (exponent 0xFF) take the
    round-to-nearest conversion instead, which keeps them inf/nan."""
    u = np.asarray(u, dtype=np.uint32)
    r16 = np.asarray(r16, dtype=np.uint32) & np.uint32(0xFFFF)
    stochastic = ((u.astype(np.uint64) + r16.astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
    special = ((u >> np.uint32(23)) & np.uint32(0xFF)) == np.uint32(0xFF)
    if special.any():
        f = torch.from_numpy(np.ascontiguousarray(u).view(np.int32).copy()).view(torch.float32)
        nearest = f.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        stochastic = np.where(special, nearest, stochastic)
    return stochastic


def stochastic_round_bf16(x, seed, step, ordinal, lane, index=None):
    """Round the fp32 tensor `x` to bf16 with the bits the kernels use.
    `index` gives each element's index within its tensor (default: its flat
    position in `x`). Runs on the CPU; the result lands on `x`'s device."""
    assert x.dtype == torch.float32, "stochastic_round_bf16 rounds float32 tensors"
    flat = x.detach().contiguous().view(-1).cpu()
    if index is None:
        index = np.arange(flat.numel(), dtype=np.uint64)
    r16 = lane_bits(element_words(seed, step, ordinal, index), lane)
    u = flat.view(torch.int32).numpy().view(np.uint32)
    out = round_bits_to_bf16(u, r16)
    out = torch.from_numpy(out.view(np.int16).copy()).view(torch.bfloat16)
    return out.view(x.shape).to(x.device)
