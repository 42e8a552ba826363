"""RoPE in the q/k/v LoRA epilogue: the vectorised q+k rope kernel against the
scalar one (bit-equal), lora_add_nt_rope_group_ against lora_add_nt_ per
sibling followed by rope_fwd (bit-equal), and lora_group_forward(..., rope=)
with RELORA_AMD_LORA_GROUP_ROPE on and off (bit-equal, one child process
each).  All @gpu.

Tolerances against the float64 composition are those of
tests/test_gpu_lora_group_bwd.py: 0.05 * max(1, |ref|max) for outputs and dx,
0.03 * |ref|max + 0.05 for dA and dB; against rope_torch the 2e-2 + 2e-2 *
max(1, |ref|) of tests/test_gpu_kernels.py.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd import ops
from relora_amd.ops import functional as Fn
from relora_amd.ops import hip
from relora_amd.ops.functional import _next_dropout_seed, set_dropout_rng_state

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lora_group_rope_worker as worker  # noqa: E402

SEED_MASK = 0x7FFFFFFFFFFFFFFF


def ext():
    return hip.ext()


def max_err(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item()


def assert_close_bf16(got, ref, atol=2e-2, rtol=2e-2, what=""):
    err = (got.float() - ref).abs()
    bad = err > (atol + rtol * ref.abs().clamp_min(1.0))
    assert not bad.any(), f"{what}: max abs err {err.max().item():.4f}"


# -- 1. vectorised rope_fwd against the scalar kernel ----------------------------

def qk(B, nh, nkv, S, hd, layout, seed):
    g = torch.Generator().manual_seed(seed)
    if layout == "bhsd":
        q = torch.randn(B, nh, S, hd, generator=g).to(torch.bfloat16).cuda()
        k = torch.randn(B, nkv, S, hd, generator=g).to(torch.bfloat16).cuda()
    else:  # transposed view of a BSHD buffer
        q = torch.randn(B, S, nh, hd, generator=g).to(torch.bfloat16).cuda().transpose(1, 2)
        k = torch.randn(B, S, nkv, hd, generator=g).to(torch.bfloat16).cuda().transpose(1, 2)
    return q, k


@pytest.mark.parametrize("layout", ["bhsd", "bshd_t"])
@pytest.mark.parametrize("B,nh,nkv,S,hd,R,cache", [
    (2, 4, 2, 96, 64, 64, 128),     # GQA, cache longer than the sequence
    (1, 2, 2, 40, 128, 128, 40),
    (1, 2, 2, 33, 64, 16, 33),      # partial rotary: the tail copy
])
def test_rope_vec_equals_scalar(B, nh, nkv, S, hd, R, cache, layout):
    q, k = qk(B, nh, nkv, S, hd, layout, seed=B + nh + S + hd + R)
    cos, sin = ops.build_rope_cache(R, cache, device="cuda")
    for inverse in (False, True):
        vq, vk = ext().rope_fwd(q, k, cos, sin, inverse)
        sq, sk = ext().rope_fwd(q, k, cos, sin, inverse, force_scalar=True)
        assert vq.stride() == q.stride() and vk.stride() == k.stride()
        assert torch.equal(vq, sq), (inverse, "q")
        assert torch.equal(vk, sk), (inverse, "k")
    vq, vk = ext().rope_fwd(q, k, cos, sin, False)
    rq, rk = ops.rope_torch(q.float(), k.float(), cos, sin)
    assert_close_bf16(vq, rq, what="q")
    assert_close_bf16(vk, rk, what="k")


def test_rope_vec_no_partner():
    """k without heads (a lone rotary sibling in the group backward)"""
    q, _ = qk(2, 4, 4, 96, 64, "bshd_t", seed=3)
    k = q.new_empty(2, 0, 96, 64)
    cos, sin = ops.build_rope_cache(64, 96, device="cuda")
    vq, vk = ext().rope_fwd(q, k, cos, sin, True)
    sq, _ = ext().rope_fwd(q, q, cos, sin, True, force_scalar=True)
    assert vk.shape == k.shape and torch.equal(vq, sq)


def test_rope_small_rotary_takes_scalar_path():
    """R/2 = 4 is no multiple of 8: the scalar kernels, still right"""
    q, k = qk(1, 2, 2, 33, 64, "bhsd", seed=9)
    cos, sin = ops.build_rope_cache(8, 33, device="cuda")
    a = ext().rope_fwd(q, k, cos, sin, False)
    b = ext().rope_fwd(q, k, cos, sin, False, force_scalar=True)
    rq, rk = ops.rope_torch(q.float(), k.float(), cos, sin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert_close_bf16(a[0], rq, what="q")
    assert_close_bf16(a[1], rk, what="k")


# -- 2. lora_add_nt_rope_group_ ----------------------------------------------------

B, S = worker.B, worker.S
M = B * S  # 192: the second 128-row tile is partial, positions wrap inside a tile


def kernel_inputs(Ns, r, seed):
    g = torch.Generator().manual_seed(seed)
    outs = [torch.randn(M, N, generator=g).to(torch.bfloat16).cuda() for N in Ns]
    Ps = [(torch.randn(M, r, generator=g) * 0.3).to(torch.bfloat16).cuda() for _ in Ns]
    Qs = [(torch.randn(N, r, generator=g) * 0.3).to(torch.bfloat16).cuda() for N in Ns]
    return outs, Ps, Qs


def heads(y, hd):
    return y.view(B, S, y.shape[1] // hd, hd).transpose(1, 2)


def unfused(outs, Ps, Qs, flags, cos, sin, hd):
    ys = [o.clone() for o in outs]
    for y, P, Q in zip(ys, Ps, Qs):
        ext().lora_add_nt_(y, P, Q)
    rot = [g for g, f in enumerate(flags) if f]
    for i in range(0, len(rot), 2):
        pair = [heads(ys[g], hd) for g in rot[i:i + 2]]
        if len(pair) == 1:
            pair.append(pair[0].new_empty(B, 0, S, hd))
        res = ext().rope_fwd(pair[0], pair[1], cos, sin, False)
        for g, y in zip(rot[i:i + 2], res):
            ys[g] = y.transpose(1, 2).reshape(M, -1)
    return ys


def reference64(outs, Ps, Qs, flags, cos, sin, hd):
    refs = []
    for o, P, Q, f in zip(outs, Ps, Qs, flags):
        y = o.cpu().double() + P.cpu().double() @ Q.cpu().double().t()
        if f:
            y4 = heads(y, hd)
            y4, _ = ops.rope_torch(y4, y4, cos.cpu().double(), sin.cpu().double())
            y = y4.transpose(1, 2).reshape(M, -1)
        refs.append(y)
    return refs


@pytest.mark.parametrize("r", [32, 128])
@pytest.mark.parametrize("hd,Ns,flags", [
    (64, (256, 128, 128), (1, 1, 0)),    # GQA
    (64, (256, 256, 256), (1, 1, 0)),
    (128, (256, 256, 256), (1, 1, 0)),
    (64, (256, 128), (1, 0)),            # G = 2
    (64, (256, 256, 256), (0, 0, 0)),    # plain lora_add_nt_
])
def test_add_nt_rope_group(hd, Ns, flags, r):
    outs, Ps, Qs = kernel_inputs(Ns, r, seed=hd + sum(Ns) + r)
    cos, sin = ops.build_rope_cache(hd, 128, device="cuda")
    want = unfused(outs, Ps, Qs, flags, cos, sin, hd)
    got = [o.clone() for o in outs]
    ext().lora_add_nt_rope_group_(got, Ps, Qs, list(flags), cos, sin, S, hd)
    refs = reference64(outs, Ps, Qs, flags, cos, sin, hd)
    for g, (a, b, ref) in enumerate(zip(got, want, refs)):
        e_got, e_want = max_err(a, ref), max_err(b, ref)
        print(f"hd {hd} Ns {Ns} r {r} sibling {g}: unfused err {e_want:.3e} "
              f"fused err {e_got:.3e} |ref|max {ref.abs().max().item():.3e}")
        assert torch.equal(a, b), g
        assert e_got <= e_want, (g, e_got, e_want)
        if any(flags) and not flags[g]:
            assert not torch.equal(a, outs[g])  # the unrotated sibling was still added to


def test_add_nt_rope_group_rejects_unsupported():
    cos, sin = ops.build_rope_cache(96, 128, device="cuda")
    outs, Ps, Qs = kernel_inputs((192,), 32, seed=1)
    with pytest.raises(RuntimeError):   # head_dim 96
        ext().lora_add_nt_rope_group_(outs, Ps, Qs, [1], cos, sin, S, 96)
    cos, sin = ops.build_rope_cache(64, 128, device="cuda")
    with pytest.raises(RuntimeError):   # N no multiple of 128
        ext().lora_add_nt_rope_group_(outs, Ps, Qs, [1], cos, sin, S, 64)
    outs, Ps, Qs = kernel_inputs((256,), 32, seed=1)
    with pytest.raises(RuntimeError):   # tables shorter than the sequence
        ext().lora_add_nt_rope_group_(outs, Ps, Qs, [1], cos[:64].contiguous(),
                                      sin[:64].contiguous(), S, 64)


# -- 3. the op, switch on and off, one child process each ---------------------------

def run_worker(tmp_path, switch):
    out = tmp_path / f"rope{switch}.pt"
    env = dict(os.environ, RELORA_AMD_LORA_GROUP_ROPE=switch)
    res = subprocess.run([sys.executable, os.path.join(HERE, "lora_group_rope_worker.py"),
                          str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def worker_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora_group_rope")
    return run_worker(d, "1"), run_worker(d, "0")


def unpack_mask(mask, rows, K):
    mb = mask.view(rows, K // 8)
    bits = torch.zeros(rows, K, device=mask.device, dtype=torch.bool)
    for j in range(8):
        bits[:, j::8] = ((mb >> j) & 1).bool()
    return bits


def op_reference(case, train):
    """float64 composition on the CPU: linear + LoRA (with the masks the philox
    stream yields in training mode), then rope_torch on the flagged outputs."""
    hd, Ns, r, flags = worker.CASES[case]
    mods = worker.make_modules(Ns, r, train)   # also sets torch's seed as the worker did
    x, dys, cos, sin = worker.make_io(Ns, hd)
    set_dropout_rng_state(worker.C0)
    x64 = x.cpu().double().requires_grad_(True)
    ys, As, Bs = [], [], []
    for m, f in zip(mods, flags):
        xd = x64
        if train:
            seed = _next_dropout_seed() & SEED_MASK
            _, mask = ext().dropout_mask_fwd(x.view(M, worker.K), worker.P, seed)
            keep = unpack_mask(mask, M, worker.K).cpu().view(B, S, worker.K)
            xd = x64 * keep.double() / (1.0 - worker.P)
        A = m.lora_A.weight.detach().cpu().double().requires_grad_(True)
        Bw = m.lora_B.weight.detach().cpu().double().requires_grad_(True)
        y = x64 @ m.weight.detach().cpu().double().t() + \
            float(m._post_lora_scale()) * (xd @ A.t()) @ Bw.t()
        if f:
            y4 = y.view(B, S, -1, hd).transpose(1, 2)
            y4, _ = ops.rope_torch(y4, y4, cos.cpu().double(), sin.cpu().double())
            y = y4.transpose(1, 2).reshape(B, S, -1)
        ys.append(y)
        As.append(A)
        Bs.append(Bw)
    torch.autograd.backward(ys, [d.cpu().double() for d in dys])
    return ([y.detach() for y in ys], x64.grad, [a.grad for a in As], [b.grad for b in Bs])


@pytest.mark.parametrize("mode", ["cases", "eval"])
@pytest.mark.parametrize("case", sorted(worker.CASES))
def test_switch_on_matches_off(worker_results, case, mode):
    on, off = worker_results
    assert on["switch"] is True and off["switch"] is False
    a, b = on[mode][case], off[mode][case]
    for key in ("ys", "dAs", "dBs"):
        for g, (ta, tb) in enumerate(zip(a[key], b[key])):
            assert torch.equal(ta, tb), (key, g)
    assert torch.equal(a["dx"], b["dx"])
    rys, rdx, rdAs, rdBs = op_reference(case, train=mode == "cases")
    for side in (a, b):
        for g, ref in enumerate(rys):
            assert max_err(side["ys"][g], ref) <= 0.05 * max(1.0, ref.abs().max().item()), g
        assert max_err(side["dx"], rdx) <= 0.05 * max(1.0, rdx.abs().max().item())
        for g, (ra, rb) in enumerate(zip(rdAs, rdBs)):
            assert max_err(side["dAs"][g], ra) <= 0.03 * ra.abs().max().item() + 0.05, g
            assert max_err(side["dBs"][g], rb) <= 0.03 * rb.abs().max().item() + 0.05, g


def test_fused_kernel_runs_only_where_it_can(worker_results):
    on, off = worker_results
    for case in worker.CASES:
        assert off["fused_calls"][case] == 0
        assert on["fused_calls"][case] == (0 if case == "hd96_fallback" else 1), case
    assert off["fused_calls"]["llama"] == 0
    assert on["fused_calls"]["llama"] == 4   # 2 models x 2 layers


@pytest.mark.parametrize("nkv", [4, 2])
def test_llama_same_loss_on_and_off(worker_results, nkv):
    on, off = worker_results
    assert torch.isfinite(on["llama"][nkv]["loss"])
    assert torch.equal(on["llama"][nkv]["loss"], off["llama"][nkv]["loss"])
    assert torch.equal(on["llama"][nkv]["dA_q0"], off["llama"][nkv]["dA_q0"])


# -- 4. position_ids keep the two separate calls --------------------------------------

def test_position_ids_do_not_take_the_fused_path(monkeypatch):
    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaAttention

    assert Fn._LORA_GROUP_ROPE
    cfg = LlamaConfig(vocab_size=128, hidden_size=256, intermediate_size=344,
                      num_hidden_layers=1, num_attention_heads=4, max_position_embeddings=128)
    attn = LlamaAttention(cfg)
    attn.q_proj, attn.k_proj, attn.v_proj = worker.make_modules((256, 256, 256), 32)
    attn = attn.to(device="cuda", dtype=torch.bfloat16).train()
    calls = []
    real = ops.lora_linear_group

    def counting(*a, **kw):
        calls.append(kw.get("rope") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "lora_linear_group", counting)
    x = torch.randn(B, S, 256, device="cuda", dtype=torch.bfloat16)
    set_dropout_rng_state(5)
    fused, _ = attn(x)
    pos = torch.arange(S, device="cuda").unsqueeze(0).expand(B, S)
    set_dropout_rng_state(5)
    plain, _ = attn(x, position_ids=pos)
    assert calls == [True, False]
    # the torch rope of the position_ids path rounds differently: close, not equal
    assert_close_bf16(fused, plain.float(), what="attention output")
