"""AdamW number formats for bf16 training, CPU side: the Philox reference,
the stochastic rounding rule, the two defects the options exist for (stalled
second moment, vanishing updates), state handling, and the trainer flags.

Statistical bounds are 6 sigma of the binomial model of the rounding rule
(each rounding goes up with probability q = low16/65536, so its error has
variance ulp^2 * q * (1 - q)), computed here from the test's own numbers."""

import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from relora_amd.ops import philox
from relora_amd.ops.optim import AdamW, adamw_reference_update

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_to_f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


# ---------------------------------------------------------------------------
# Philox reference
# ---------------------------------------------------------------------------


def test_philox_known_answers():
    """Random123 known-answer vectors for philox4x32-10."""
    w = philox.philox4x32_10((0, 0), (0, 0, 0, 0))
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    w = philox.philox4x32_10((ones, ones), (ones, ones, ones, ones))
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    w = philox.philox4x32_10((0xA4093822, 0x299F31D0),
                             (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344))
    assert [int(x) for x in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_philox_counter_layout():
    """element_words puts (index lo, index hi, step, ordinal) in the counter
    and the halves of the seed in the key."""
    seed = 0x0123456789ABCDEF
    idx = np.array([5, (7 << 32) + 9], dtype=np.uint64)
    got = philox.element_words(seed, 11, 13, idx)
    for j, (lo, hi) in enumerate([(5, 0), (9, 7)]):
        want = philox.philox4x32_10((0x89ABCDEF, 0x01234567), (lo, hi, 11, 13))
        assert [int(w[j]) for w in got] == [int(w) for w in want]
    # a negative seed is its two's-complement 64-bit pattern
    a = philox.element_words(-1, 1, 0, idx)
    b = philox.element_words(0xFFFFFFFFFFFFFFFF, 1, 0, idx)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_philox_distinct_counters_distinct_words():
    idx = np.arange(64, dtype=np.uint64)
    seen = set()
    for step in (1, 2, 3):
        for ordinal in (0, 1, 2):
            w = philox.element_words(7, step, ordinal, idx)
            for j in range(64):
                seen.add(tuple(int(x[j]) for x in w))
    assert len(seen) == 3 * 3 * 64
    # ... and the first two words alone (the ones the lanes read) differ too
    assert len({t[:2] for t in seen}) == 3 * 3 * 64
    # another seed moves everything
    w7 = philox.element_words(7, 1, 0, idx)
    w8 = philox.element_words(8, 1, 0, idx)
    assert not np.any(w7[0] == w8[0])


def test_lane_bits():
    words = (np.array([0xABCD1234], dtype=np.uint32), np.array([0x5678EF01], dtype=np.uint32),
             np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    assert int(philox.lane_bits(words, philox.LANE_PARAM)[0]) == 0x1234
    assert int(philox.lane_bits(words, philox.LANE_EXP_AVG)[0]) == 0xABCD
    assert int(philox.lane_bits(words, philox.LANE_EXP_AVG_SQ)[0]) == 0xEF01
    with pytest.raises(ValueError):
        philox.lane_bits(words, 3)


# ---------------------------------------------------------------------------
# rounding rule on hand-built bit patterns
# ---------------------------------------------------------------------------


def test_rounding_exact_values_never_move():
    u = np.array([0x3F800000, 0xBF800000, 0x00000000, 0x80000000, 0x3F810000, 0x00010000,
                  0x7F7F0000], dtype=np.uint32)
    for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
        out = philox.round_bits_to_bf16(u, np.full(u.shape, r, dtype=np.uint32))
        assert np.array_equal(out, (u >> 16).astype(np.uint16)), hex(r)


def test_rounding_half_goes_up_iff_r_at_least_half():
    u = np.array([0x3F808000], dtype=np.uint32)  # halfway between 0x3F80 and 0x3F81
    for r, want in ((0, 0x3F80), (0x7FFF, 0x3F80), (0x8000, 0x3F81), (0xFFFF, 0x3F81)):
        assert int(philox.round_bits_to_bf16(u, np.array([r], dtype=np.uint32))[0]) == want
    # low16 = 1 goes up only for r = 0xFFFF; low16 = 0xFFFF for every r >= 1
    u = np.array([0x3F800001, 0x3F80FFFF], dtype=np.uint32)
    assert list(philox.round_bits_to_bf16(u, np.array([0xFFFE, 0], np.uint32))) == [0x3F80, 0x3F80]
    assert list(philox.round_bits_to_bf16(u, np.array([0xFFFF, 1], np.uint32))) == [0x3F81, 0x3F81]


def test_rounding_negative_rounds_in_magnitude():
    u = np.array([0xBF808000], dtype=np.uint32)  # -(1 + 2^-8)
    down = philox.round_bits_to_bf16(u, np.array([0x7FFF], dtype=np.uint32))
    up = philox.round_bits_to_bf16(u, np.array([0x8000], dtype=np.uint32))
    assert int(down[0]) == 0xBF80 and int(up[0]) == 0xBF81  # -1.0 / -1.0078125
    # denormals follow the same rule, and carry into the smallest normal
    u = np.array([0x00008000, 0x807FFFFF], dtype=np.uint32)
    assert list(philox.round_bits_to_bf16(u, np.array([0x8000, 1], np.uint32))) == [0x0001, 0x8080]


def test_rounding_inf_nan_pass_through_and_carry_to_inf():
    u = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
    for r in (0, 0xFFFF):
        out = philox.round_bits_to_bf16(u, np.full(u.shape, r, dtype=np.uint32))
        assert int(out[0]) == 0x7F80 and int(out[1]) == 0xFF80
        back = torch.from_numpy(out.view(np.int16).copy()).view(torch.bfloat16)
        assert torch.isnan(back[2:]).all()  # nan stays nan, never becomes inf
    # largest finite bf16 plus a carry is inf, as round-to-nearest would give
    u = np.array([0x7F7F8000, 0xFF7FFFFF], dtype=np.uint32)
    out = philox.round_bits_to_bf16(u, np.array([0x8000, 1], dtype=np.uint32))
    assert list(out) == [0x7F80, 0xFF80]
    out = philox.round_bits_to_bf16(u, np.array([0x7FFF, 0], dtype=np.uint32))
    assert list(out) == [0x7F7F, 0xFF7F]


@pytest.mark.parametrize("lane", [0, 1, 2])
def test_stochastic_round_is_unbiased(lane):
    """One fp32 value rounded 2^20 times with different counters: the mean
    error is inside 6 sigma of the binomial model."""
    n = 1 << 20
    x = bits_to_f32([0x3F8D3B71])  # 1.1034985..., low16 = 0x3B71
    q = 0x3B71 / 65536.0
    ulp = 2.0 ** -7  # bf16 spacing in [1, 2)
    out = philox.stochastic_round_bf16(x.expand(n).contiguous(), seed=3, step=17, ordinal=5,
                                       lane=lane)
    lo, hi = bits_to_f32([0x3F8D0000]).item(), bits_to_f32([0x3F8E0000]).item()
    vals = out.double()
    assert set(vals.unique().tolist()) == {lo, hi}
    mean_err = (vals.mean() - x.double().item()).item()
    sigma = ulp * math.sqrt(q * (1 - q) / n)
    print(f"lane {lane}: mean error {mean_err:.3e}, sigma {sigma:.3e}")
    assert abs(mean_err) <= 6 * sigma


def test_public_op_cpu_path_and_validation():
    from relora_amd import ops

    x = torch.randn(1000)
    a = ops.stochastic_round_bf16(x, 1, 2, 3, 0)
    assert a.dtype == torch.bfloat16 and a.shape == x.shape
    assert torch.equal(a, philox.stochastic_round_bf16(x, 1, 2, 3, 0))
    assert ((a.float() - x).abs() <= (x.abs() * 2.0 ** -7)).all()
    with pytest.raises(ValueError):
        ops.stochastic_round_bf16(x.double(), 1, 2, 3, 0)
    with pytest.raises(ValueError):
        ops.stochastic_round_bf16(x, 1, 2, 3, 3)


# ---------------------------------------------------------------------------
# the two defects
# ---------------------------------------------------------------------------


def _second_moment_reference(g, beta2, steps):
    """float64 recursion with the hyperparameter as the fp32 kernels see it."""
    b2 = float(np.float32(beta2))
    one_minus = float(np.float32(1) - np.float32(beta2))
    v = 0.0
    for _ in range(steps):
        v = b2 * v + one_minus * g * g
    return v


def _run_constant_grad(n_elem, steps, g_value, p_value, **opt_kwargs):
    p = torch.nn.Parameter(torch.full((n_elem,), p_value, dtype=torch.bfloat16))
    g = torch.full((n_elem,), g_value, dtype=torch.bfloat16)
    opt = AdamW([p], **opt_kwargs)
    for _ in range(steps):
        p.grad = g
        opt.step()
    return p, opt.state[p]


def test_second_moment_stalls_in_bf16_and_not_with_the_options():
    """g == const, beta2 = 0.999, 2000 steps: bf16 moments with nearest
    rounding stop tracking g^2 (the defect); fp32 moments follow the float64
    recursion; stochastic rounding follows it in the mean."""
    steps, n = 2000, 4096
    g = torch.tensor(0.37, dtype=torch.bfloat16).item()  # 0.369140625
    ref = _second_moment_reference(g, 0.999, steps)
    kw = dict(lr=0.0, betas=(0.9, 0.999), weight_decay=0.0)

    _, st = _run_constant_grad(n, steps, g, 0.5, **kw)
    assert st["exp_avg_sq"].dtype == torch.bfloat16
    stalled = st["exp_avg_sq"].double().mean().item()
    gap = abs(stalled - ref) / ref
    print(f"bf16 nearest: v = {stalled:.6f}, reference {ref:.6f}, gap {gap:.1%}")
    assert gap > 0.10

    _, st = _run_constant_grad(n, steps, g, 0.5, state_dtype=torch.float32, **kw)
    assert st["exp_avg_sq"].dtype == torch.float32
    # each step rounds twice (product, sum), each within 2^-24 of a value <= ref,
    # and an error made k steps ago has decayed by beta2^k: sum <= 2^-23 / (1 - beta2)
    fp32_bound = ref * 2.0 ** -23 / (1 - 0.999)
    err = (st["exp_avg_sq"].double() - ref).abs().max().item()
    print(f"fp32 moments: max error {err:.3e} (bound {fp32_bound:.3e})")
    assert err <= fp32_bound

    _, st = _run_constant_grad(n, steps, g, 0.5, rounding="stochastic", rounding_seed=11, **kw)
    assert st["exp_avg_sq"].dtype == torch.bfloat16
    # each step adds an independent, zero-mean rounding error of variance
    # ulp^2 q(1-q) <= ulp^2 / 4 (ulp taken at the final, largest value), which
    # decays by beta2 per later step: var <= ulp^2/4 * sum beta2^(2k)
    ulp = 2.0 ** (math.floor(math.log2(ref)) - 7)
    var_elem = ulp ** 2 / 4 * sum(0.999 ** (2 * k) for k in range(steps))
    sigma = math.sqrt(var_elem / n)
    mean_err = st["exp_avg_sq"].double().mean().item() - ref
    print(f"stochastic: mean error {mean_err:.3e}, sigma {sigma:.3e}, fp32 term {fp32_bound:.3e}")
    assert abs(mean_err) <= 6 * sigma + fp32_bound
    assert 6 * sigma + fp32_bound < 0.01 * ref  # the band itself is tight against the 10 % gap


def test_small_updates_vanish_with_nearest_and_survive_stochastic():
    """Parameters at 0.75 with lr = 1e-4: every update is under half a bf16
    ulp (2^-9), so nearest rounding never moves them; stochastic rounding
    moves them by n * lr in the mean."""
    steps, n, lr = 1000, 65536, 1e-4
    kw = dict(lr=lr, betas=(0.9, 0.999), weight_decay=0.0, state_dtype=torch.float32)

    p, _ = _run_constant_grad(n, steps, 1.0, 0.75, **kw)
    assert torch.equal(p.detach(), torch.full((n,), 0.75, dtype=torch.bfloat16))

    p, st = _run_constant_grad(n, steps, 1.0, 0.75, rounding="stochastic", rounding_seed=5, **kw)
    assert st["exp_avg"].dtype == torch.float32
    # constant gradient: m_hat / (sqrt(v_hat) + eps) = 1 up to fp32 rounding, so
    # every step asks for -lr. The parameter stays in [0.5, 1): ulp = 2^-8.
    ulp = 2.0 ** -8
    q = lr / ulp
    sigma = ulp * math.sqrt(steps * q * (1 - q) / n)
    # p - lr is itself rounded to fp32 (half an fp32 ulp of [0.5, 1) per step)
    fp32_term = steps * 2.0 ** -25
    displacement = 0.75 - p.detach().double().mean().item()
    print(f"mean displacement {displacement:.6f} (n*lr = {steps * lr:.6f}), sigma {sigma:.3e}, "
          f"6 sigma {6 * sigma:.3e}, fp32 term {fp32_term:.3e}")
    assert p.detach().min().item() >= 0.5
    assert abs(displacement - steps * lr) <= 6 * sigma + fp32_term


# ---------------------------------------------------------------------------
# options, ordinals, state handling
# ---------------------------------------------------------------------------


def test_option_validation():
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError):
        AdamW(p, state_dtype=torch.float16)
    with pytest.raises(ValueError):
        AdamW(p, state_dtype="float32")
    with pytest.raises(ValueError):
        AdamW(p, rounding="random")
    with pytest.raises(ValueError):
        AdamW(p, rounding_seed=1.5)
    with pytest.raises(ValueError):
        AdamW(p, rounding_seed=1 << 63)
    AdamW(p, state_dtype=torch.float32, rounding="stochastic", rounding_seed=-1)


def test_ordinals_follow_construction_order_and_extend():
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(5)]
    opt = AdamW([{"params": ps[:2]}, {"params": ps[2:4], "lr": 1e-2}])
    assert [opt.ordinal(p) for p in ps[:4]] == [0, 1, 2, 3]
    opt.add_param_group({"params": [ps[4]]})
    assert [opt.ordinal(p) for p in ps] == [0, 1, 2, 3, 4]


def _params(dtype, seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n).to(dtype)) for n in (7, 300, 1025)]


def _steps(opt, params, n, seed=1):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)
        opt.step()


def test_ordinal_feeds_the_counter():
    """Two parameters with identical data draw different bits, and the bits
    are the reference's for (seed, step, ordinal, index)."""
    base = torch.randn(512).bfloat16()
    ps = [torch.nn.Parameter(base.clone()) for _ in range(2)]
    opt = AdamW(ps, lr=1e-3, weight_decay=0.0, rounding="stochastic", rounding_seed=9,
                state_dtype=torch.float32)
    g = torch.randn(512).bfloat16()
    want = []
    for o, p in enumerate(ps):
        new_p, _, _ = adamw_reference_update(p, g, torch.zeros(512), torch.zeros(512), lr=1e-3,
                                             beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1)
        want.append(philox.stochastic_round_bf16(new_p, 9, 1, o, philox.LANE_PARAM))
        p.grad = g
    opt.step()
    assert torch.equal(ps[0].detach(), want[0]) and torch.equal(ps[1].detach(), want[1])
    assert not torch.equal(ps[0].detach(), ps[1].detach())


def test_state_dict_round_trip_keeps_fp32_moments_and_ordinals():
    params = _params(torch.bfloat16)
    kw = dict(lr=1e-2, state_dtype=torch.float32, rounding="stochastic", rounding_seed=4)
    opt = AdamW(params, **kw)
    _steps(opt, params, 3)
    sd = opt.state_dict()
    # through a file, as a checkpoint goes
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)

    params2 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = AdamW(params2, **kw)
    opt2.load_state_dict(sd)
    for p, p2 in zip(params, params2):
        assert opt.ordinal(p) == opt2.ordinal(p2)
        for key in ("exp_avg", "exp_avg_sq"):
            assert opt2.state[p2][key].dtype == torch.float32
            assert torch.equal(opt2.state[p2][key], opt.state[p][key])
        assert opt2.state[p2]["step"] == opt.state[p]["step"]
    # and the next step is bit-identical
    _steps(opt, params, 1, seed=2)
    _steps(opt2, params2, 1, seed=2)
    for p, p2 in zip(params, params2):
        assert torch.equal(p.detach(), p2.detach())
        assert torch.equal(opt.state[p]["exp_avg_sq"], opt2.state[p2]["exp_avg_sq"])


def test_cross_loading_between_state_dtypes():
    params = _params(torch.bfloat16)
    # bf16-moment checkpoint -> fp32-moment optimizer: exact upcast
    opt_bf16 = AdamW(params, lr=1e-2)
    _steps(opt_bf16, params, 2)
    opt_f32 = AdamW(params, lr=1e-2, state_dtype=torch.float32)
    opt_f32.load_state_dict(opt_bf16.state_dict())
    for p in params:
        for key in ("exp_avg", "exp_avg_sq"):
            assert opt_f32.state[p][key].dtype == torch.float32
            assert torch.equal(opt_f32.state[p][key], opt_bf16.state[p][key].float())
    # fp32-moment checkpoint -> default optimizer: round-to-nearest downcast
    _steps(opt_f32, params, 2)
    opt_back = AdamW(params, lr=1e-2)
    opt_back.load_state_dict(opt_f32.state_dict())
    for p in params:
        for key in ("exp_avg", "exp_avg_sq"):
            assert opt_back.state[p][key].dtype == torch.bfloat16
            assert torch.equal(opt_back.state[p][key], opt_f32.state[p][key].bfloat16())
    # the loaded copies do not alias the checkpoint
    sd = opt_f32.state_dict()
    opt_f32b = AdamW(params, lr=1e-2, state_dtype=torch.float32)
    opt_f32b.load_state_dict(sd)
    assert opt_f32b.state[params[0]]["exp_avg"].data_ptr() != sd["state"][0]["exp_avg"].data_ptr()


@pytest.mark.parametrize("mode", ["zero", "random", "magnitude"])
@pytest.mark.parametrize("wrapped", [False, True])
def test_optimizer_reset_keeps_moment_dtype(mode, wrapped):
    from relora_amd.parallel import ZeroRedundancyAdamW
    from relora_amd.training_utils import optimizer_reset

    params = _params(torch.bfloat16)
    kw = dict(lr=1e-2, state_dtype=torch.float32, rounding="stochastic")
    opt = ZeroRedundancyAdamW(params, **kw) if wrapped else AdamW(params, **kw)
    _steps(opt, params, 2)
    inner = opt.optim if wrapped else opt
    assert inner.state_dtype == torch.float32 and inner.rounding == "stochastic"
    optimizer_reset(
        opt, reset_params=params, optimizer_state_keys=["exp_avg", "exp_avg_sq"],
        reset_optimizer_on_relora=mode == "zero",
        optimizer_random_pruning=0.5 if mode == "random" else 0.0,
        optimizer_magnitude_pruning=0.5 if mode == "magnitude" else 0.0,
    )
    for p in params:
        for key in ("exp_avg", "exp_avg_sq"):
            t = inner.state[p][key]
            assert t.dtype == torch.float32
            if p.numel() > 100:
                assert (t == 0).float().mean() > 0.3
    _steps(opt, params, 1)
    assert all(inner.state[p]["exp_avg"].dtype == torch.float32 for p in params)


def test_zero_wrapper_passes_options_and_keeps_fp32_state():
    from relora_amd.parallel import ZeroRedundancyAdamW

    params = _params(torch.bfloat16)
    kw = dict(lr=1e-2, state_dtype=torch.float32, rounding="stochastic", rounding_seed=3)
    opt = ZeroRedundancyAdamW(params, **kw)
    assert (opt.optim.state_dtype, opt.optim.rounding, opt.optim.rounding_seed) == \
        (torch.float32, "stochastic", 3)
    assert [opt.optim.ordinal(p) for p in params] == [0, 1, 2]
    _steps(opt, params, 2)
    opt.consolidate_state_dict()
    sd = opt.state_dict()
    assert all(st[k].dtype == torch.float32 for st in sd["state"].values()
               for k in ("exp_avg", "exp_avg_sq"))
    # (on the CPU the consolidated dict shares storage with the live state)
    opt2 = ZeroRedundancyAdamW(params, **kw)
    opt2.load_state_dict(copy.deepcopy(sd))
    for p in params:
        for key in ("exp_avg", "exp_avg_sq"):
            assert opt2.optim.state[p][key].dtype == torch.float32
            assert torch.equal(opt2.optim.state[p][key], opt.optim.state[p][key])
    # the same wrapper steps exactly like the plain optimizer (same ordinals)
    plain_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    plain = AdamW(plain_params, **kw)
    plain.load_state_dict(copy.deepcopy(sd))
    _steps(opt2, params, 1, seed=5)
    _steps(plain, plain_params, 1, seed=5)
    for p, q in zip(params, plain_params):
        assert torch.equal(p.detach(), q.detach())


def _parent_adamw_steps(params, n, *, lr, betas, eps, wd, seed=1):
    """The optimizer step as it was before the options existed, inlined."""
    state = {}
    gen = torch.Generator().manual_seed(seed)
    beta1, beta2 = betas
    for _ in range(n):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)
        with torch.no_grad():
            ps, gs, ms, vs, steps = [], [], [], [], []
            for p in params:
                if p not in state:
                    state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p),
                                "exp_avg_sq": torch.zeros_like(p)}
                state[p]["step"] += 1
                ps.append(p)
                gs.append(p.grad)
                ms.append(state[p]["exp_avg"])
                vs.append(state[p]["exp_avg_sq"])
                steps.append(int(state[p]["step"].item()))
            if wd != 0:
                torch._foreach_mul_(ps, 1 - lr * wd)
            torch._foreach_lerp_(ms, gs, 1 - beta1)
            torch._foreach_mul_(vs, beta2)
            torch._foreach_addcmul_(vs, gs, gs, 1 - beta2)
            for p, m, v, s in zip(ps, ms, vs, steps):
                bc1 = 1 - beta1 ** s
                bc2 = 1 - beta2 ** s
                denom = (v.float() / bc2).sqrt_().add_(eps)
                p.data.add_(((-lr / bc1) * m.float() / denom).to(p.dtype))
    return state


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_defaults_are_bit_identical_to_the_plain_optimizer(dtype):
    hp = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
    a = _params(dtype)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt = AdamW(a, weight_decay=0.01, **hp)
    _steps(opt, a, 5)
    state = _parent_adamw_steps(b, 5, wd=0.01, **hp)
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
        for key in ("exp_avg", "exp_avg_sq"):
            assert opt.state[p][key].dtype == dtype
            assert torch.equal(opt.state[p][key], state[q][key])
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}


def test_fp32_parameters_ignore_the_options():
    a = _params(torch.float32)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt = AdamW(a, lr=1e-2, state_dtype=torch.float32, rounding="stochastic")
    ref = AdamW(b, lr=1e-2)
    _steps(opt, a, 3)
    _steps(ref, b, 3)
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


def test_reference_update_float64_agrees_with_float32():
    torch.manual_seed(0)
    p, g = torch.randn(4096).bfloat16(), torch.randn(4096).bfloat16()
    m, v = torch.randn(4096) * 0.1, torch.rand(4096) * 0.1
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.01, step=3)
    lo = adamw_reference_update(p, g, m, v, **kw)
    hi = adamw_reference_update(p, g, m, v, math_dtype=torch.float64, **kw)
    for a, b in zip(lo, hi):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.allclose(a.double(), b, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------


def _run_args(tmp_path, extra=None, steps=6):
    from relora_amd.trainer import parse_args

    base = [
        "--model_config", "configs/llama_9m.json",
        "--synthetic_data", "true",
        "--use_peft", "true",
        "--relora", "3", "--cycle_length", "3",
        "--restart_warmup_steps", "1",
        "--scheduler", "cosine_restarts",
        "--warmup_steps", "2",
        "--num_training_steps", str(steps),
        "--batch_size", "2", "--total_batch_size", "4",
        "--max_length", "32",
        "--lr", "1e-3", "--dtype", "bfloat16",
        "--eval_every", "100", "--save_every", "100",
        "--workers", "0",
        "--save_dir", str(tmp_path / "run"),
    ]
    return parse_args(base + (extra or []))


@pytest.fixture
def single_proc_env(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    yield
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


BOTH_ON = ["--adam_state_dtype", "float32", "--adam_rounding", "stochastic"]


def test_trainer_flags_parse_and_validate(tmp_path):
    args = _run_args(tmp_path)
    assert (args.adam_state_dtype, args.adam_rounding) == ("param", "nearest")
    assert args.adam_rounding_seed == args.seed == 0
    args = _run_args(tmp_path, extra=BOTH_ON + ["--seed", "17"])
    assert (args.adam_state_dtype, args.adam_rounding, args.adam_rounding_seed) == \
        ("float32", "stochastic", 17)
    args = _run_args(tmp_path, extra=BOTH_ON + ["--seed", "17", "--adam_rounding_seed", "99"])
    assert args.adam_rounding_seed == 99
    with pytest.raises(ValueError):
        _run_args(tmp_path, extra=["--adam_state_dtype", "float16"])
    with pytest.raises(ValueError):
        _run_args(tmp_path, extra=["--adam_rounding", "up"])


@pytest.mark.parametrize("optimizer", ["adam", "adam_zero"])
def test_trainer_flags_reach_the_optimizer(tmp_path, monkeypatch, single_proc_env, optimizer):
    from relora_amd import trainer

    built = []

    class Recording(AdamW):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    monkeypatch.setattr(trainer, "AdamW", Recording)
    import relora_amd.parallel.zero as zero
    monkeypatch.setattr(zero, "AdamW", Recording)
    trainer.main(_run_args(tmp_path, steps=3, extra=BOTH_ON + [
        "--adam_rounding_seed", "21", "--optimizer", optimizer, "--save_every", "3"]))
    assert len(built) == 1
    opt = built[0]
    assert (opt.state_dtype, opt.rounding, opt.rounding_seed) == (torch.float32, "stochastic", 21)
    ckpt = torch.load(tmp_path / "run" / "model_3" / "optimizer.pt", map_location="cpu",
                      weights_only=False)
    cfg = ckpt["config"]
    assert (cfg["adam_state_dtype"], cfg["adam_rounding"], cfg["adam_rounding_seed"]) == \
        ("float32", "stochastic", 21)
    assert ckpt["optimizer"]["state"]
    for st in ckpt["optimizer"]["state"].values():
        assert st["exp_avg"].dtype == torch.float32 and st["exp_avg_sq"].dtype == torch.float32
    weights = torch.load(tmp_path / "run" / "model_3" / "pytorch_model.bin", map_location="cpu",
                         weights_only=True)
    assert all(w.dtype == torch.bfloat16 for k, w in weights.items() if "lora_" in k)


def test_trainer_float32_accepts_the_flags(tmp_path, single_proc_env):
    from relora_amd import trainer

    trainer.main(_run_args(tmp_path, steps=3, extra=BOTH_ON + ["--dtype", "float32"]))
    assert (tmp_path / "run" / "model_3" / "optimizer.pt").exists()


def test_resume_is_bit_exact_with_both_options(tmp_path, single_proc_env):
    """Stop at step 3 and resume to 6 with fp32 moments and stochastic
    rounding on: weights and moments equal the uninterrupted run's, because
    the random bits depend on (seed, step, ordinal, index) alone."""
    import torch.distributed as dist

    from relora_amd.trainer import main

    extra = BOTH_ON + ["--save_every", "3", "--seed", "5"]
    main(_run_args(tmp_path / "full", extra=extra, steps=6))
    if dist.is_initialized():
        dist.destroy_process_group()
    main(_run_args(tmp_path / "half", extra=extra, steps=3))
    if dist.is_initialized():
        dist.destroy_process_group()
    main(_run_args(tmp_path / "half", extra=extra + ["--autoresume", "true"], steps=6))

    def load(run, name, **kw):
        return torch.load(tmp_path / run / "run" / "model_6" / name, map_location="cpu", **kw)

    a = load("full", "pytorch_model.bin", weights_only=True)
    b = load("half", "pytorch_model.bin", weights_only=True)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa = load("full", "optimizer.pt", weights_only=False)["optimizer"]["state"]
    sb = load("half", "optimizer.pt", weights_only=False)["optimizer"]["state"]
    assert set(map(str, sa)) == set(map(str, sb)) and sa
    for k in sa:
        for key in ("exp_avg", "exp_avg_sq"):
            assert sa[k][key].dtype == torch.float32
            assert torch.equal(sa[k][key], sb[k][key]), (k, key)
    # the rounding did something: another rounding seed gives other weights
    main(_run_args(tmp_path / "other", extra=extra + ["--adam_rounding_seed", "6"], steps=6))
    c = torch.load(tmp_path / "other" / "run" / "model_6" / "pytorch_model.bin",
                   map_location="cpu", weights_only=True)
    assert any(not torch.equal(a[k], c[k]) for k in a)


@pytest.mark.timeout(900)
def test_torchrun_two_proc_zero_fp32_moments(tmp_path):
    """gloo world-2 `adam_zero` run with fp32 moments: the consolidated
    checkpoint holds them as fp32, and a resumed run reloads them as fp32
    and carries on."""
    keep = ("PATH", "HOME", "TMPDIR", "LD_LIBRARY_PATH", "ROCM_PATH",
            "HSA_ENABLE_IPC_MODE_LEGACY", "PYTHONPATH", "HIP_VISIBLE_DEVICES")
    env = {k: os.environ[k] for k in keep if k in os.environ}
    env["RELORA_AMD_NO_TQDM"] = "1"
    env["OMP_NUM_THREADS"] = "1"
    env["CUDA_VISIBLE_DEVICES"] = ""  # a CPU/gloo test wherever it runs
    env["HIP_VISIBLE_DEVICES"] = ""

    def launch(steps, more, tag):
        cmd = [
            sys.executable, "-m", "torch.distributed.run",
            "--standalone", "--local-addr", "127.0.0.1",
            "--nnodes=1", "--nproc-per-node=2",
            "torchrun_main.py",
            "--model_config", "configs/llama_9m.json",
            "--synthetic_data", "true",
            "--use_peft", "true", "--optimizer", "adam_zero",
            "--relora", "2", "--cycle_length", "2",
            "--restart_warmup_steps", "1", "--warmup_steps", "1",
            "--scheduler", "cosine_restarts",
            "--num_training_steps", str(steps),
            "--batch_size", "2", "--total_batch_size", "8",
            "--max_length", "32", "--lr", "1e-3", "--dtype", "bfloat16",
            "--eval_every", "100", "--save_every", "2", "--workers", "0",
            "--save_dir", str(tmp_path / "run"),
        ] + BOTH_ON + more
        out_path = tmp_path / f"torchrun_{tag}.out"
        with open(out_path, "w") as out:
            res = subprocess.run(cmd, cwd=REPO, env=env, stdin=subprocess.DEVNULL, stdout=out,
                                 stderr=subprocess.STDOUT, timeout=400, start_new_session=True)
        assert res.returncode == 0, out_path.read_text()[-2500:]
        return out_path.read_text()

    def moments(step):
        ckpt = torch.load(tmp_path / "run" / f"model_{step}" / "optimizer.pt",
                          map_location="cpu", weights_only=False)
        state = ckpt["optimizer"]["state"]
        assert state
        for st in state.values():
            assert st["exp_avg"].dtype == torch.float32
            assert st["exp_avg_sq"].dtype == torch.float32
        return state

    launch(2, [], "first")
    first = moments(2)
    log = launch(4, ["--autoresume", "true"], "resumed")
    state = json.load(open(tmp_path / "run" / "model_4" / "training_state.json"))
    assert state["update_step"] == 4
    resumed = moments(4)
    assert set(first) == set(resumed)
    assert "AdamW number formats: state_dtype=float32, rounding=stochastic" in log
