"""GPU tests of the AdamW number-format kernels (`fused_adamw_ex`,
`stochastic_round_bf16`) against the Python reference in
`relora_amd.ops.philox` and the CPU path of the optimizer.

Bounds: fp32 destinations use the plain kernel's bound (`atol=1e-5`,
allclose defaults, `test_fused_adamw_matches_torch_gpu`). A bf16 destination
is a bf16 neighbour of the kernel's fp32 value, so it lies within one bf16
ulp of the float64 reference value, plus the rounding error of the kernel's
own fp32 arithmetic, bounded a priori from the operand magnitudes (a few
2^-24 of the terms; about 2^-16 ulp). Up/down decisions are compared with
the reference fed the CPU path's fp32 value: they agree except where an
fp32 contraction difference straddles a rounding boundary, about 1 element
in 65536 per differing fp32 ulp; the tests require more than 99 %."""

import math

import numpy as np
import pytest
import torch

from relora_amd.ops import philox
from relora_amd.ops.optim import AdamW, adamw_reference_update

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
HP = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.01)
SEED = 0x1234_5678_9ABC
INSTANTIATIONS = [
    pytest.param(torch.bfloat16, True, id="bf16-sr"),
    pytest.param(torch.float32, False, id="f32-nearest"),
    pytest.param(torch.float32, True, id="f32-sr"),
]


def ext():
    from relora_amd.ops import hip

    return hip.ext_or_raise()


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.int64)


def bf16_ulp(x):
    """bf16 spacing at |x| (float64 tensor); the denormal spacing below 2^-126."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def make_state(numels, moment_dtype, seed=0, device="cuda"):
    """Random parameters, grads and moments; exp_avg shares the grad's sign so
    the first-moment update does not cancel (the ulp bound is relative)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    ps, gs, ms, vs = [], [], [], []
    for n in numels:
        r = lambda: torch.randn(n, device=device, generator=gen)  # noqa: E731
        ps.append(r().bfloat16())
        g = r()
        gs.append(g.bfloat16())
        ms.append((g.sign() * r().abs() * 0.1).to(moment_dtype))
        vs.append((r().square() * 0.1).to(moment_dtype))
    return ps, gs, ms, vs


def run_ex(ps, gs, ms, vs, *, step, stochastic, seed=SEED, ordinals=None):
    ps, ms, vs = ([t.clone() for t in ts] for ts in (ps, ms, vs))
    ordinals = list(range(len(ps))) if ordinals is None else ordinals
    ext().fused_adamw_ex(ps, gs, ms, vs, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                         HP["wd"], step, stochastic, seed, ordinals)
    torch.cuda.synchronize()
    return ps, ms, vs


def check_region(before, after, *, lo, hi, step, ordinal, stochastic, seed=SEED):
    """Compare elements [lo, hi) of one tensor with the references, which are
    evaluated at those indices only. Returns (matching, compared) decisions."""
    p0, g0, m0, v0 = (t[lo:hi].cpu() for t in before)
    p1, m1, v1 = (t[lo:hi].cpu() for t in after)
    kw = dict(step=step, **HP)
    ref64 = adamw_reference_update(p0, g0, m0, v0, math_dtype=torch.float64, **kw)
    ref32 = adamw_reference_update(p0, g0, m0, v0, math_dtype=torch.float32, **kw)
    index = np.arange(lo, hi, dtype=np.uint64)
    words = philox.element_words(seed, step, ordinal, index) if stochastic else None

    # a priori fp32 evaluation error of each destination (see module docstring)
    m_mag = m0.double().abs() + g0.double().abs()
    v_mag = v0.double().abs() + g0.double().square()
    bc1 = 1 - HP["beta1"] ** step
    bc2 = 1 - HP["beta2"] ** step
    denom = (ref64[2] / bc2).sqrt() + HP["eps"]
    fp32_err = {
        philox.LANE_PARAM: 8 * EPS32 * (p0.double().abs() + HP["lr"] / bc1 * m_mag / denom),
        philox.LANE_EXP_AVG: 4 * EPS32 * m_mag,
        philox.LANE_EXP_AVG_SQ: 4 * EPS32 * v_mag,
    }

    matching = compared = 0
    for out, r64, r32, lane in ((p1, ref64[0], ref32[0], philox.LANE_PARAM),
                                (m1, ref64[1], ref32[1], philox.LANE_EXP_AVG),
                                (v1, ref64[2], ref32[2], philox.LANE_EXP_AVG_SQ)):
        if out.dtype == torch.float32:
            assert torch.allclose(out, r64.float(), atol=1e-5), (lane, (out - r64).abs().max())
            continue
        ulp = bf16_ulp(torch.maximum(r64.abs(), out.double().abs()))
        err = (out.double() - r64).abs()
        worst = (err - ulp - fp32_err[lane]).max().item()
        assert worst <= 0, f"lane {lane}: {worst:.3e} beyond one bf16 ulp of the reference"
        if stochastic:
            want = philox.round_bits_to_bf16(
                r32.contiguous().view(torch.int32).numpy().view(np.uint32),
                philox.lane_bits(words, lane)).astype(np.int64)
        else:
            want = bits16(r32.bfloat16())
        diff = np.abs(bits16(out) - want)
        matching += int((diff == 0).sum())
        compared += diff.size
    return matching, compared


def check_tensors(before, after, which, *, step, stochastic, ordinals=None, window=None):
    matching = compared = 0
    for t in which:
        n = before[0][t].numel()
        regions = [(0, n)] if window is None or n <= 2 * window else \
            [(0, window), (n - window, n)]
        for lo, hi in regions:
            a, b = check_region([ts[t] for ts in before], [ts[t] for ts in after], lo=lo, hi=hi,
                                step=step, ordinal=t if ordinals is None else ordinals[t],
                                stochastic=stochastic)
            matching += a
            compared += b
    if compared:
        share = matching / compared
        print(f"decisions equal to the reference: {matching}/{compared} = {share:.4%}")
        assert share > 0.99
    return matching, compared


# ---------------------------------------------------------------------------
# stochastic_round_bf16
# ---------------------------------------------------------------------------


def value_mix(n, seed):
    """Normals over many binades, denormals, both signs, bf16-exact values,
    inf and nan, cycled to length n."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen) * torch.pow(2.0, torch.randint(-40, 40, (n,), generator=gen))
    special = torch.tensor([0x00000001, 0x80000001, 0x00008000, 0x007FFFFF, 0x807FFFFF,  # denormal
                            0x3F800000, 0xBF810000, 0x00000000, 0x80000000,  # exact
                            0x3F808000, 0xBF80FFFF, 0x3F800001,  # half, nearly up, nearly down
                            0x7F7FFFFF, 0xFF7F8000, 0x7F7F0000,  # largest finite
                            0xFF800000, 0x7F800000, 0x7FC00000, 0x7F800001],  # inf, nan
                           dtype=torch.int64)
    special = (special & 0xFFFFFFFF).numpy().astype(np.uint32).view(np.int32)
    special = torch.from_numpy(special.copy()).view(torch.float32)
    pos = torch.arange(0, n, 3)[: special.numel()]
    x[pos] = special[: pos.numel()]
    return x


@pytest.mark.parametrize("lane", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 255, 257, 65535, 65537])
def test_stochastic_round_bit_equal_to_reference(n, lane):
    from relora_amd import ops

    x = value_mix(n, seed=n)
    for step, ordinal in ((1, 0), (70000, 513)):
        got = ops.stochastic_round_bf16(x.cuda(), SEED, step, ordinal, lane).cpu()
        want = philox.stochastic_round_bf16(x, SEED, step, ordinal, lane)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        nan = torch.isnan(x)
        assert torch.equal(torch.isnan(got), nan)
        assert np.array_equal(bits16(got)[~nan.numpy()], bits16(want)[~nan.numpy()])


def test_stochastic_round_all_special_values_present():
    x = value_mix(257, seed=257)
    assert torch.isnan(x).sum() >= 2 and torch.isinf(x).sum() >= 2
    assert ((x != 0) & (x.abs() < 2.0 ** -126)).sum() >= 5


# ---------------------------------------------------------------------------
# fused_adamw_ex against the CPU path
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("moment_dtype,stochastic", INSTANTIATIONS)
@pytest.mark.parametrize("n", [1, 255, 257, 65536, 65537])
def test_fused_adamw_ex_single_tensor(n, moment_dtype, stochastic):
    before = make_state([n], moment_dtype, seed=n)
    after = run_ex(*before, step=3, stochastic=stochastic, ordinals=[7])
    check_tensors(before, after, [0], step=3, stochastic=stochastic, ordinals=[7])


@pytest.mark.parametrize("moment_dtype,stochastic", INSTANTIATIONS)
def test_fused_adamw_ex_fifty_tensors_two_tables(moment_dtype, stochastic):
    """50 small tensors: more than MT_MAX = 48, so two chunk tables."""
    numels = [17 + 31 * i for i in range(50)]
    before = make_state(numels, moment_dtype, seed=50)
    after = run_ex(*before, step=2, stochastic=stochastic)
    check_tensors(before, after, range(50), step=2, stochastic=stochastic)


@pytest.mark.parametrize("moment_dtype,stochastic", INSTANTIATIONS)
def test_fused_adamw_ex_list_crossing_320_chunks(moment_dtype, stochastic):
    """12 tensors of 30 chunks each (29 full + 1 element): the eleventh no
    longer fits the first table's 320 blocks. Every tensor's first and last
    4096 elements are compared."""
    numels = [29 * 65536 + 1] * 12
    before = make_state(numels, moment_dtype, seed=320)
    after = run_ex(*before, step=5, stochastic=stochastic)
    check_tensors(before, after, range(12), step=5, stochastic=stochastic, window=4096)


@pytest.mark.parametrize("moment_dtype,stochastic", INSTANTIATIONS)
def test_single_tensor_kernel_uses_the_global_index(moment_dtype, stochastic):
    """One tensor just above 320 chunks takes the grid-stride kernel; a
    3-chunk tensor in the same call takes the chunk table. Both must use the
    element's index within its tensor: compared at the first and last 4096
    elements and the 4096 around index 65536, the reference evaluated only
    there."""
    big = 320 * 65536 + 1
    before = make_state([big, 2 * 65536 + 5], moment_dtype, seed=321)
    after = run_ex(*before, step=4, stochastic=stochastic, ordinals=[3, 9])
    matching = compared = 0
    for t, n, ordinal in ((0, big, 3), (1, 2 * 65536 + 5, 9)):
        for lo, hi in ((0, 4096), (65536 - 2048, 65536 + 2048), (n - 4096, n)):
            a, b = check_region([ts[t] for ts in before], [ts[t] for ts in after], lo=lo, hi=hi,
                                step=4, ordinal=ordinal, stochastic=stochastic)
            matching += a
            compared += b
    if compared:
        print(f"decisions equal to the reference: {matching}/{compared}")
        assert matching / compared > 0.99
    # the middle of the big tensor was updated too (grid-stride covers it all)
    mid = slice(big // 2, big // 2 + 4096)
    assert not torch.equal(before[0][0][mid], after[0][0][mid])


def test_determinism_and_counter_sensitivity():
    before = make_state([70000, 300], torch.bfloat16, seed=9)
    base = run_ex(*before, step=3, stochastic=True)
    again = run_ex(*before, step=3, stochastic=True)
    for a, b in zip(base, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    other_seed = run_ex(*before, step=3, stochastic=True, seed=SEED + 1)
    other_ordinal = run_ex(*before, step=3, stochastic=True, ordinals=[5, 6])
    for other in (other_seed, other_ordinal):
        for t in range(2):
            assert not torch.equal(base[0][t], other[0][t])
            assert not torch.equal(base[2][t], other[2][t])
            # same fp32 values, other bits: still neighbours of each other
            assert np.abs(bits16(base[0][t]) - bits16(other[0][t])).max() <= 1
    # another step changes the bias corrections as well; compare the bits alone
    x = torch.randn(70000, device="cuda")
    a = ext().stochastic_round_bf16(x, SEED, 3, 0, 0)
    assert torch.equal(a, ext().stochastic_round_bf16(x, SEED, 3, 0, 0))
    for seed, step, ordinal, lane in ((SEED + 1, 3, 0, 0), (SEED, 4, 0, 0), (SEED, 3, 1, 0),
                                      (SEED, 3, 0, 1), (SEED, 3, 0, 2)):
        assert not torch.equal(a, ext().stochastic_round_bf16(x, seed, step, ordinal, lane))


def _spy(monkeypatch):
    calls = []
    real = {name: getattr(ext(), name) for name in ("fused_adamw", "fused_adamw_ex")}
    for name, fn in real.items():
        def wrapper(*a, _name=name, _fn=fn, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(ext(), name, wrapper)
    return calls


def _step_once(dtype, **opt_kwargs):
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n, device="cuda").to(dtype)) for n in (300, 70000)]
    opt = AdamW(params, lr=1e-2, **opt_kwargs)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    torch.cuda.synchronize()
    return params, opt


def test_defaults_call_the_plain_kernel_only(monkeypatch):
    calls = _spy(monkeypatch)
    _step_once(torch.bfloat16)
    _step_once(torch.bfloat16, state_dtype=None, rounding="nearest")
    # fp32 parameters: nothing to round, moments already fp32
    _step_once(torch.float32, state_dtype=torch.float32, rounding="stochastic")
    assert calls and set(calls) == {"fused_adamw"}


@pytest.mark.parametrize("opt_kwargs", [
    dict(state_dtype=torch.float32), dict(rounding="stochastic"),
    dict(state_dtype=torch.float32, rounding="stochastic")])
def test_options_call_the_ex_kernel_only(monkeypatch, opt_kwargs):
    calls = _spy(monkeypatch)
    params, opt = _step_once(torch.bfloat16, **opt_kwargs)
    assert calls == ["fused_adamw_ex"]
    want = torch.float32 if "state_dtype" in opt_kwargs else torch.bfloat16
    for p in params:
        assert p.dtype == torch.bfloat16 and opt.state[p]["exp_avg"].dtype == want
        assert torch.isfinite(p).all()


@pytest.mark.parametrize("moment_dtype,stochastic", INSTANTIATIONS)
def test_optimizer_gpu_step_matches_its_cpu_path(moment_dtype, stochastic):
    """The public optimizer, three steps on the GPU and on the CPU from the
    same start: the GPU state after each step, fed to the CPU path, gives the
    same next state up to the bounds above (so no drift is compared)."""
    kw = dict(lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"],
              weight_decay=HP["wd"], rounding="stochastic" if stochastic else "nearest",
              state_dtype=torch.float32 if moment_dtype == torch.float32 else None,
              rounding_seed=SEED)
    torch.manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(n, device="cuda").bfloat16()) for n in (257, 66000)]
    opt = AdamW(params, **kw)
    for step in (1, 2, 3):
        grads = [torch.randn_like(p) for p in params]
        if step == 1:
            zeros = [torch.zeros_like(p, dtype=moment_dtype) for p in params]
            before = ([p.detach().clone() for p in params], grads, zeros, zeros)
        else:
            before = ([p.detach().clone() for p in params], grads,
                      [opt.state[p]["exp_avg"].clone() for p in params],
                      [opt.state[p]["exp_avg_sq"].clone() for p in params])
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
        after = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params],
                 [opt.state[p]["exp_avg_sq"] for p in params])
        assert after[1][0].dtype == moment_dtype
        check_tensors(before, after, range(2), step=step, stochastic=stochastic)


# ---------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------


def _call(ps, gs, ms, vs, stochastic=True, ordinals=None):
    ext().fused_adamw_ex(ps, gs, ms, vs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, stochastic, 0,
                         list(range(len(ps))) if ordinals is None else ordinals)


def test_host_checks():
    def t(n=64, dtype=torch.bfloat16, device="cuda"):
        return torch.zeros(n, dtype=dtype, device=device)

    with pytest.raises(RuntimeError, match="share a dtype"):  # mixed moment dtypes
        _call([t(), t()], [t(), t()], [t(), t(dtype=torch.float32)], [t(), t(dtype=torch.float32)])
    with pytest.raises(RuntimeError, match="share a dtype"):
        _call([t()], [t()], [t()], [t(dtype=torch.float32)])
    with pytest.raises(RuntimeError, match="bfloat16"):  # fp32 parameters
        f = torch.float32
        _call([t(dtype=f)], [t(dtype=f)], [t(dtype=f)], [t(dtype=f)])
    with pytest.raises(RuntimeError, match="numel"):
        _call([t(64)], [t(64)], [t(63)], [t(64)])
    with pytest.raises(RuntimeError, match="numel"):
        _call([t(64)], [t(32)], [t(64)], [t(64)])
    with pytest.raises(RuntimeError, match="contiguous"):
        _call([t(128)[::2]], [t(64)], [t(64)], [t(64)])
    with pytest.raises(RuntimeError, match="contiguous"):
        _call([t(64)], [t(64)], [t(64, dtype=torch.float32)],
              [t(128, dtype=torch.float32)[::2]], stochastic=False)
    with pytest.raises(RuntimeError, match="GPU|device"):  # wrong device
        _call([t(device="cpu")], [t(device="cpu")], [t(device="cpu")], [t(device="cpu")])
    with pytest.raises(RuntimeError, match="device"):
        _call([t()], [t()], [t(device="cpu")], [t()])
    with pytest.raises(RuntimeError, match="one entry per tensor"):
        _call([t()], [t()], [t()], [t()], ordinals=[0, 1])
    with pytest.raises(RuntimeError, match="plain fused_adamw"):  # (bf16, nearest) never routes here
        _call([t()], [t()], [t()], [t()], stochastic=False)
    with pytest.raises(RuntimeError, match="float32"):
        ext().stochastic_round_bf16(t(), 0, 1, 0, 0)
    with pytest.raises(RuntimeError, match="lane"):
        ext().stochastic_round_bf16(t(dtype=torch.float32), 0, 1, 0, 3)
    # nothing above launched anything; an empty call is a no-op
    _call([], [], [], [])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------


def test_relora_llama_trains_with_both_options():
    """2-layer LLaMA (hidden 256) under ReLoRA, 20 steps with fp32 moments
    and stochastic rounding: the loss goes down, dtypes are as asked, and a
    merge-and-reset cycle through optimizer_reset leaves them alone."""
    from relora_amd.models import build_model_from_config
    from relora_amd.models.config import LlamaConfig
    from relora_amd.relora import ReLoRaModel
    from relora_amd.training_utils import optimizer_reset

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=688,
                      num_hidden_layers=2, num_attention_heads=4,
                      max_position_embeddings=128, rms_norm_eps=1e-6)
    model = ReLoRaModel(build_model_from_config(cfg), r=32, lora_alpha=32, lora_dropout=0.0,
                        target_modules=["attn", "attention", "mlp"], keep_original_weights=True)
    model = model.to(device="cuda", dtype=torch.bfloat16).train()
    trainable = [p for p in model.parameters() if p.requires_grad]
    lora = [p for n, p in model.named_parameters() if p.requires_grad and "lora_" in n]
    assert lora
    opt = AdamW(trainable, lr=2e-3, weight_decay=0.0, state_dtype=torch.float32,
                rounding="stochastic", rounding_seed=1)
    x = torch.randint(0, cfg.vocab_size, (4, 64), device="cuda")

    def dtypes_ok():
        for p in trainable:
            assert p.dtype == torch.bfloat16
            st = opt.state[p]
            assert st["exp_avg"].dtype == torch.float32
            assert st["exp_avg_sq"].dtype == torch.float32
            assert torch.isfinite(p).all()

    losses = []
    for step in range(20):
        loss = model(input_ids=x, labels=x).loss
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
        if step == 9:  # one merge-and-reset cycle
            dtypes_ok()
            model.merge_and_reinit()
            optimizer_reset(opt, reset_params=lora,
                            optimizer_state_keys=["exp_avg", "exp_avg_sq"],
                            reset_optimizer_on_relora=True, optimizer_random_pruning=0.0,
                            optimizer_magnitude_pruning=0.0)
            dtypes_ok()
            assert (opt.state[lora[0]]["exp_avg"] == 0).float().mean() > 0.9
    dtypes_ok()
    print("losses:", [round(v, 3) for v in losses])
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0] - 0.1
