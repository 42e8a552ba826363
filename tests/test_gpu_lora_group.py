"""Group LoRA linear (lora_down_dropout kernel, lora_group_fwd/bwd, the
relora.lora_group_forward helper) vs the single-linear path and float64 CPU
references.  All @gpu."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd import ops
from relora_amd.ops import hip
from relora_amd.ops import functional as Fn
from relora_amd.ops.functional import (_next_dropout_seed, get_dropout_rng_state,
                                       lora_linear, lora_linear_group,
                                       set_dropout_rng_state)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_MASK = 0x7FFFFFFFFFFFFFFF


def ext():
    return hip.ext()


def unpack_mask(mask, M, K):
    mb = mask.view(M, K // 8)
    bits = torch.zeros(M, K, device=mask.device, dtype=torch.bool)
    for j in range(8):
        bits[:, j::8] = ((mb >> j) & 1).bool()
    return bits


def make_down_inputs(M, K, r, G, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    As = [(torch.randn(r, K, generator=g) * 0.1).to(torch.bfloat16).cuda()
          for _ in range(G)]
    seeds = [(0x1234567 * (i + 1) + seed) & SEED_MASK for i in range(G)]
    return x, As, seeds


DOWN_SHAPES = [(256, 64, 32, 1), (130, 72, 64, 2), (257, 200, 128, 3),
               (64, 2048, 256, 3)]


# -- 1. masks ---------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,K,r,G", DOWN_SHAPES)
def test_masks_bit_identical(M, K, r, G, p):
    x, As, seeds = make_down_inputs(M, K, r, G, seed=M + K)
    out = ext().lora_down_dropout(x, As, seeds, p)
    assert len(out) == 2 * G
    for g in range(G):
        _, ref_mask = ext().dropout_mask_fwd(x, p, seeds[g])
        assert out[G + g].shape == ref_mask.shape
        assert torch.equal(out[G + g], ref_mask), f"sibling {g}"


# -- 2. t_g numerics ---------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,K,r,G", DOWN_SHAPES)
def test_down_projection_numerics(M, K, r, G, p):
    """Bound: twice the library path's own max abs error against the float64
    reference on the same inputs, floored at one bf16 ulp of the largest
    output magnitude (a different fp32 summation order, nothing else)."""
    x, As, seeds = make_down_inputs(M, K, r, G, seed=M + K + 1)
    out = ext().lora_down_dropout(x, As, seeds, p)
    for g in range(G):
        xd, _ = ext().dropout_mask_fwd(x, p, seeds[g])
        ref = xd.cpu().double() @ As[g].cpu().double().t()
        lib = torch.nn.functional.linear(xd, As[g])
        lib_err = (lib.cpu().double() - ref).abs().max().item()
        ker_err = (out[g].cpu().double() - ref).abs().max().item()
        # bf16 has 8 significant bits: ulp of a value in [2^e, 2^(e+1)) is 2^(e-7)
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().max())).item() - 7)
        bound = max(2.0 * lib_err, ulp)
        print(f"shape {(M, K, r, G)} p {p} sibling {g}: library err {lib_err:.3e} "
              f"kernel err {ker_err:.3e} ulp {ulp:.3e}")
        assert ker_err <= bound, (
            f"sibling {g}: kernel err {ker_err:.4e} > bound {bound:.4e} "
            f"(library err {lib_err:.4e}, ulp {ulp:.4e})")


@pytest.mark.parametrize("M,K,r,G", DOWN_SHAPES)
def test_down_projection_p0(M, K, r, G):
    x, As, _ = make_down_inputs(M, K, r, G, seed=M + K + 2)
    out = ext().lora_down_dropout(x, As, [], 0.0)
    assert len(out) == G  # no mask is produced
    for g in range(G):
        ref = x.cpu().double() @ As[g].cpu().double().t()
        lib_err = (torch.nn.functional.linear(x, As[g]).cpu().double() - ref).abs().max().item()
        ker_err = (out[g].cpu().double() - ref).abs().max().item()
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().max())).item() - 7)
        assert ker_err <= max(2.0 * lib_err, ulp), (ker_err, lib_err, ulp)


def test_down_projection_rejects_unsupported():
    x, As, seeds = make_down_inputs(16, 64, 32, 1, seed=3)
    with pytest.raises(RuntimeError):
        ext().lora_down_dropout(x[:, :60].contiguous(), [As[0][:, :60].contiguous()],
                                seeds, 0.1)                       # K % 8 != 0
    with pytest.raises(RuntimeError):
        ext().lora_down_dropout(x, [As[0][:16].contiguous()], seeds, 0.1)   # r % 32
    with pytest.raises(RuntimeError):
        ext().lora_down_dropout(x, As * 4, seeds * 4, 0.1)        # G > 3


# -- 3. group fwd/bwd vs sequential calls and a float64 reference -------------

def make_group(M, K, Ns, r, seed, zero_w=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    specs = []
    for N in Ns:
        W = (torch.randn(N, K, generator=g) * (0.0 if zero_w else 0.05))
        A = torch.randn(r, K, generator=g) * 0.05
        B = torch.randn(N, r, generator=g) * 0.05
        specs.append([t.to(torch.bfloat16).cuda() for t in (W, A, B)])
    dys = [torch.randn(M, N, generator=g).to(torch.bfloat16).cuda() for N in Ns]
    return x, specs, dys


def run_group(x, specs, dys, scale, p, c0):
    x = x.detach().clone().requires_grad_(True)
    leaves = [[W, A.detach().clone().requires_grad_(True),
               B.detach().clone().requires_grad_(True)] for W, A, B in specs]
    set_dropout_rng_state(c0)
    ys = lora_linear_group(x, [(W, None, A, B, scale) for W, A, B in leaves],
                           dropout_p=p, training=True)
    torch.autograd.backward(ys, dys)
    return ys, x.grad, [l[1].grad for l in leaves], [l[2].grad for l in leaves]


def run_sequential(x, specs, dys, scale, p, c0):
    x = x.detach().clone().requires_grad_(True)
    leaves = [[W, A.detach().clone().requires_grad_(True),
               B.detach().clone().requires_grad_(True)] for W, A, B in specs]
    set_dropout_rng_state(c0)
    ys = [lora_linear(x, W, None, A, B, scale, dropout_p=p, training=True)
          for W, A, B in leaves]
    torch.autograd.backward(ys, dys)
    return ys, x.grad, [l[1].grad for l in leaves], [l[2].grad for l in leaves]


def run_reference(x, specs, dys, scale, p, c0):
    """float64 on the CPU, with the masks the philox stream yields from c0."""
    M, K = x.shape
    set_dropout_rng_state(c0)
    seeds = [_next_dropout_seed() & SEED_MASK for _ in specs]
    x64 = x.cpu().double().requires_grad_(True)
    ys, As, Bs, keeps = [], [], [], []
    for (W, A, B), seed in zip(specs, seeds):
        _, mask = ext().dropout_mask_fwd(x, p, seed)
        keep = unpack_mask(mask, M, K).cpu()
        keeps.append(keep)
        A64 = A.cpu().double().requires_grad_(True)
        B64 = B.cpu().double().requires_grad_(True)
        xd = x64 * keep.double() / (1.0 - p)
        ys.append(x64 @ W.cpu().double().t() + scale * (xd @ A64.t()) @ B64.t())
        As.append(A64)
        Bs.append(B64)
    torch.autograd.backward(ys, [d.cpu().double() for d in dys])
    return ([y.detach() for y in ys], x64.grad, [a.grad for a in As],
            [b.grad for b in Bs], keeps)


def check_against(got, ref, what):
    ys, dx, dAs, dBs = got
    rys, rdx, rdAs, rdBs = ref[:4]

    def close(a, b, tol, name):
        err = (a.detach().cpu().double() - b).abs().max().item()
        assert err <= tol, f"{what} {name}: err {err:.4e} > tol {tol:.4e}"

    for g in range(len(ys)):
        close(ys[g], rys[g], 0.05 * max(1.0, rys[g].abs().max().item()), f"y[{g}]")
        close(dAs[g], rdAs[g], 0.03 * rdAs[g].abs().max().item() + 0.05, f"dA[{g}]")
        close(dBs[g], rdBs[g], 0.03 * rdBs[g].abs().max().item() + 0.05, f"dB[{g}]")
    close(dx, rdx, 0.05 * max(1.0, rdx.abs().max().item()), "dx")


GROUP_CASES = {
    "aligned_g3": dict(M=192, K=256, Ns=(256, 256, 256), r=64),   # lora_add_nt_
    "odd_n_g2": dict(M=192, K=256, Ns=(333, 333), r=64),          # addmm_, library dB
    "fused_k1": dict(M=256, K=256, Ns=(256, 256), r=64),          # fused_lora_gemm
    # r % 64 == 32: the transposed tile of lora_add_nn_ holds a partial
    # 64-element rotation block per row
    "aligned_g3_r32": dict(M=192, K=256, Ns=(256, 256, 256), r=32),
    "odd_n_g2_r96": dict(M=192, K=256, Ns=(333, 333), r=96),
}


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_group_matches_sequential_and_reference(case):
    c = GROUP_CASES[case]
    scale, p, c0 = 0.5, 0.1, 1000
    x, specs, dys = make_group(c["M"], c["K"], c["Ns"], c["r"], seed=21)
    if case == "fused_k1":
        assert Fn._use_fused_k1(x, specs[0][0], specs[0][1])
    else:
        assert not Fn._use_fused_k1(x, specs[0][0], specs[0][1])
    ref = run_reference(x, specs, dys, scale, p, c0)
    check_against(run_sequential(x, specs, dys, scale, p, c0), ref, "sequential")
    check_against(run_group(x, specs, dys, scale, p, c0), ref, "group")
    assert get_dropout_rng_state() == c0 + len(specs)


def test_group_p0_and_eval():
    x, specs, dys = make_group(192, 256, (256, 333), 64, seed=22)
    ref = run_reference(x, specs, dys, 0.5, 0.0, 7)
    check_against(run_group(x, specs, dys, 0.5, 0.0, 7), ref, "group p=0")
    assert get_dropout_rng_state() == 7  # no seed drawn without dropout
    ys = lora_linear_group(x, [(W, None, A, B, 0.5) for W, A, B in specs],
                           dropout_p=0.1, training=False)
    assert get_dropout_rng_state() == 7
    for y, ry in zip(ys, ref[0]):
        assert (y.cpu().double() - ry).abs().max() <= 0.05 * max(1.0, ry.abs().max().item())


def test_group_dx_respects_every_mask():
    """W = 0 isolates the LoRA part of dx: it must be exactly zero where all
    three masks drop, and follow each sibling's mask elsewhere."""
    p, c0 = 0.5, 50
    x, specs, dys = make_group(256, 512, (384, 384, 384), 64, seed=23, zero_w=True)
    ref = run_reference(x, specs, dys, 1.0, p, c0)
    _, dx, _, _ = run_group(x, specs, dys, 1.0, p, c0)
    keeps = ref[4]
    all_dropped = ~(keeps[0] | keeps[1] | keeps[2])
    dxc = dx.cpu()
    assert abs(all_dropped.float().mean().item() - p ** 3) < 0.02
    assert (dxc[all_dropped] == 0).all()
    assert (dxc[~all_dropped] != 0).float().mean() > 0.99
    check_against(run_group(x, specs, dys, 1.0, p, c0), ref, "group W=0")


@pytest.mark.parametrize("r", [32, 96, 160, 224])
@pytest.mark.parametrize("masked", [False, True])
def test_lora_add_nn_partial_rotation_block(r, masked):
    """dx += mask/(1-p) * (u @ A) at ranks that are not a multiple of 64,
    with an M and an N tail.  Bound: the one test_gpu_lora.py applies to
    lora_add_nn_ (0.05 absolute at these magnitudes)."""
    g = torch.Generator().manual_seed(40 + r)
    M, K, p = 200, 328, 0.1
    dx0 = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    u = (torch.randn(M, r, generator=g) * 0.1).to(torch.bfloat16).cuda()
    A = (torch.randn(r, K, generator=g) * 0.1).to(torch.bfloat16).cuda()
    if masked:
        _, mask = ext().dropout_mask_fwd(dx0, p, 7)
        bits = unpack_mask(mask, M, K)
        inv_keep = 1.0 / (1.0 - p)
    else:
        mask = torch.empty(0, device="cuda", dtype=torch.uint8)
        bits = torch.ones(M, K, device="cuda", dtype=torch.bool)
        inv_keep = 1.0
    dx = dx0.clone()
    ext().lora_add_nn_(dx, u, A, mask, inv_keep)
    lora = (u.double() @ A.double()) * inv_keep
    ref = dx0.double() + torch.where(bits, lora, torch.zeros_like(lora))
    err = (dx.double() - ref).abs().max().item()
    assert err < 0.05, err


# -- 4. RNG stream -----------------------------------------------------------

def test_rng_stream_matches_sequential(monkeypatch):
    x, specs, dys = make_group(130, 72, (64, 64, 64), 32, seed=24)
    recorded = []
    real = ext().dropout_mask_fwd

    def recording(*a):
        out = real(*a)
        recorded.append(out[1].clone())
        return out

    monkeypatch.setattr(ext(), "dropout_mask_fwd", recording)
    W, A, B = specs[0]

    set_dropout_rng_state(300)
    lora_linear_group(x, [(W_, None, A_, B_, 0.5) for W_, A_, B_ in specs],
                      dropout_p=0.1, training=True)
    assert get_dropout_rng_state() == 303
    assert not recorded  # the group op has its own fused dropout
    lora_linear(x, W, None, A, B, 0.5, dropout_p=0.1, training=True)
    after_group = recorded.pop()
    assert get_dropout_rng_state() == 304

    set_dropout_rng_state(300)
    for W_, A_, B_ in specs:
        lora_linear(x, W_, None, A_, B_, 0.5, dropout_p=0.1, training=True)
    assert get_dropout_rng_state() == 303
    del recorded[:]
    lora_linear(x, W, None, A, B, 0.5, dropout_p=0.1, training=True)
    assert torch.equal(after_group, recorded.pop())


# -- 5. fallbacks -------------------------------------------------------------

def make_modules(K, Ns, rs, dtype=torch.bfloat16, **kw):
    from relora_amd.relora import ReLoRaLinear

    torch.manual_seed(31)
    mods = []
    for N, r in zip(Ns, rs):
        m = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=0.1, bias=False, **kw)
        with torch.no_grad():
            if kw.get("quantize") is None:
                m.weight.normal_(std=0.05)
            m.lora_A.weight.normal_(std=0.05)
            m.lora_B.weight.normal_(std=0.05)
        mods.append(m.to(device="cuda", dtype=dtype).train())
    return mods


@pytest.fixture
def group_counter(monkeypatch):
    calls = []
    real = ops.lora_linear_group

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "lora_linear_group", counting)
    return calls


def helper_vs_modules(x, mods):
    from relora_amd.relora import lora_group_forward

    set_dropout_rng_state(70)
    torch.manual_seed(5)  # the fp32 fallback draws from torch's generator
    got = lora_group_forward(x, mods)
    set_dropout_rng_state(70)
    torch.manual_seed(5)
    want = [m(x) for m in mods]
    return got, want


def test_helper_enters_group_op(group_counter):
    mods = make_modules(64, (64, 64, 64), (32, 32, 32))
    x = torch.randn(40, 64, device="cuda", dtype=torch.bfloat16)
    got, want = helper_vs_modules(x, mods)
    assert len(group_counter) == 1
    for a, b in zip(got, want):
        assert (a.float() - b.float()).abs().max() <= 0.05 * max(1.0, b.float().abs().max().item())


@pytest.mark.parametrize("why", ["quantized", "tensor_scale", "r_differs", "k_odd",
                                 "fp32", "forward_hook", "pre_hook", "r_256"])
def test_helper_falls_back(why, group_counter):
    K, dtype, kw, rs = 64, torch.bfloat16, {}, (32, 32)
    if why == "quantized":
        kw = dict(quantize="4bit")
    elif why == "tensor_scale":
        kw = dict(trainable_scaling=True)
    elif why == "r_differs":
        rs = (32, 64)
    elif why == "r_256":   # measured slower than the per-linear path
        rs = (256, 256)
    elif why == "k_odd":
        K = 65
    elif why == "fp32":
        dtype = torch.float32
    mods = make_modules(K, (64, 64), rs, dtype=dtype, **kw)
    if why == "forward_hook":
        mods[1].register_forward_hook(lambda m, i, o: None)
    elif why == "pre_hook":
        mods[0].register_forward_pre_hook(lambda m, i: None)
    x = torch.randn(40, K, device="cuda", dtype=dtype)
    got, want = helper_vs_modules(x, mods)
    assert not group_counter
    for a, b in zip(got, want):
        assert torch.equal(a, b)  # same per-module path, same seeds


# -- 5 (switch) and 6. model level, one child process per setting -------------

def run_worker(tmp_path, group):
    out = tmp_path / f"group{group}.pt"
    env = dict(os.environ, RELORA_AMD_LORA_GROUP=group)
    res = subprocess.run([sys.executable, os.path.join(HERE, "lora_group_worker.py"),
                          str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def worker_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora_group")
    return run_worker(d, "1"), run_worker(d, "0")


def test_env_switch_disables_grouping(worker_results):
    on, off = worker_results
    # 2 layers x (q/k/v + gate/up) x (1 fwd/bwd + 3 steps + 1 eval)
    assert on["entered"] == 2 * 2 * 5
    assert off["entered"] == 0


def test_model_grouping_on_matches_off(worker_results):
    on, off = worker_results
    assert abs(on["loss"] - off["loss"]) <= 0.05 * max(1.0, abs(off["loss"]))
    assert on["grads"].keys() == off["grads"].keys() and on["grads"]
    for name, ref in off["grads"].items():
        got = on["grads"][name]
        assert torch.isfinite(got).all(), name
        tol = 0.03 * ref.abs().max().item() + 0.05
        err = (got - ref).abs().max().item()
        assert err <= tol, name
        # the absolute floor above dwarfs gradients of this size, so also
        # bound the error relative to the tensor: 0.05 * |ref|max, the grad
        # tolerance of test_gpu_lora.py without its floor of 1
        assert err <= 0.05 * ref.abs().max().item(), (name, err, ref.abs().max().item())
    for res in (on, off):
        assert res["losses"][-1] < res["losses"][0], res["losses"]
