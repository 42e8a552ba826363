"""Grouped-query attention on the HIP kernels: `attn_fwd`/`attn_bwd` with
k, v of shape [B, nkv, S, hd], nkv dividing nh; query head h reads kv head
h // (nh // nkv).

Reference: float64 causal attention on the CPU with K/V expanded by
`repeat_interleave`, dK/dV summed back over each group in float64
(gqa_common.ref_gqa).  Bounds are the project's: err <= tol + tol*max(1,|ref|)
with tol 2e-2 for out, 3e-2 for dq/dk/dv, and 1e-2 absolute for lse.
tests/test_gqa_models.py checks on the CPU that the bf16-rounded computation
itself stays inside these bounds on the same inputs.
"""

import functools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import attn_variant_worker as aw
import gqa_common as gc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "attn_gqa_worker.py")

B, NH = 2, 4


def ext():
    from relora_amd.ops import hip

    e = hip.ext()
    assert e is not None, "HIP extension not built"
    return e


@functools.lru_cache(maxsize=None)
def case(nkv, S, hd):
    """inputs and reference, computed once and shared (never modified)"""
    q, k, v, dout = gc.make_inputs(B, NH, nkv, S, hd)
    return (q, k, v, dout), gc.ref_gqa(q, k, v, dout)


def run(q, k, v, dout):
    got = aw.run_kernels(ext(), q, k, v, dout)
    torch.cuda.synchronize()
    return got


# (a) shape grid: every new code path at its smallest shape ------------------

@pytest.mark.parametrize("S", [80, 320])
@pytest.mark.parametrize("hd", [64, 128, 40])
@pytest.mark.parametrize("nkv", [1, 2])
def test_shape_grid(nkv, hd, S):
    (q, k, v, dout), ref = case(nkv, S, hd)
    got = run(*(t.cuda() for t in (q, k, v, dout)))
    assert got["o"].shape == q.shape and got["dq"].shape == q.shape
    assert got["lse"].shape == (B, NH, S)
    assert got["dk"].shape == k.shape and got["dv"].shape == v.shape
    r = aw.all_ratios(got, ref)
    print(f"gqa nkv{nkv} hd{hd} S{S} err/bound: {r}")
    assert not gc.failures(r), r


# (b) layouts: q and kv each BHSD or transposed-BSHD -------------------------

@pytest.mark.parametrize("hd", [64, 128])
def test_layouts(hd):
    (q, k, v, dout), ref = case(2, 320, hd)
    base = run(*(t.cuda() for t in (q, k, v, dout)))
    for q_t in (False, True):
        for kv_t in (False, True):
            qq = gc.to_layout(q.cuda(), q_t)
            kk, vv = gc.to_layout(k.cuda(), kv_t), gc.to_layout(v.cuda(), kv_t)
            if q_t or kv_t:   # ld = hd on both sides only when both are BHSD
                assert qq.stride(2) != kk.stride(2)
            got = run(qq, kk, vv, dout.cuda())
            assert got["dk"].stride() == kk.stride() and got["dv"].stride() == kk.stride()
            assert got["o"].stride() == qq.stride() and got["dq"].stride() == qq.stride()
            r = aw.all_ratios(got, ref)
            print(f"gqa layout hd{hd} q_t={q_t} kv_t={kv_t} err/bound: {r}")
            assert not gc.failures(r), (q_t, kv_t, r)
            for n in ("o", "lse", "dq", "dk", "dv"):
                assert torch.equal(got[n], base[n]), (q_t, kv_t, n)


# (c) nkv == nh is the plain multi-head call ----------------------------------

@pytest.mark.parametrize("hd", [64, 128])
def test_nkv_equals_nh(hd):
    (q, k, v, dout), ref = case(NH, 320, hd)
    got = run(*(t.cuda() for t in (q, k, v, dout)))
    r = aw.all_ratios(got, ref)
    print(f"gqa nkv==nh hd{hd} err/bound: {r}")
    assert not gc.failures(r), r
    # the same inputs with q and kv in different layouts take the kv-strided
    # instantiations at n_rep == 1: bit-identical to the multi-head kernels
    got2 = run(q.cuda(), gc.to_layout(k.cuda(), True), gc.to_layout(v.cuda(), True),
               dout.cuda())
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(got2[n], got[n]), n


# (d) environment-selected instantiations, one fresh child each --------------

VARIANT_FLAGS = ("RELORA_AMD_ATTN_FWD", "RELORA_AMD_ATTN_BWD", "RELORA_AMD_ATTN_OCC4",
                 "RELORA_AMD_ATTN_TR_FWD", "RELORA_AMD_ATTN_TR_DKDV",
                 "RELORA_AMD_DQ_4WAVE", "RELORA_AMD_DQ_OCC4")
VARIANTS = {
    "v2_fwd_bwd": ({"RELORA_AMD_ATTN_FWD": "2", "RELORA_AMD_ATTN_BWD": "2"}, ["--hd128"]),
    "occ4_off_tr_fwd_off": ({"RELORA_AMD_ATTN_OCC4": "0",
                             "RELORA_AMD_ATTN_TR_FWD": "0"}, []),
    "tr_dkdv_dq4wave": ({"RELORA_AMD_ATTN_TR_DKDV": "1", "RELORA_AMD_DQ_4WAVE": "1"}, []),
    "tr_fwd_off_dq_occ4": ({"RELORA_AMD_ATTN_TR_FWD": "0", "RELORA_AMD_DQ_OCC4": "1"}, []),
}
# same budget as the variant children of test_gpu_attention_edges.py (3.5 s
# measured mean wall time, interpreter start and GPU init; limit 5x)
CHILD_TIMEOUT_S = 17.5

_casualty = None  # first child that ended without a result: no more launches


def _lost(name, how, tail=""):
    global _casualty
    _casualty = f"{name} ({how})"
    pytest.fail(f"gqa variant child {_casualty}; output tail:\n{tail[-2000:]}")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_child(name):
    if _casualty is not None:
        pytest.fail(f"not launched: gqa variant child {_casualty} went down first")
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:
        _lost("(none launched)", f"this process's GPU context is in error: {ex}")
    flags, extra = VARIANTS[name]
    env = {k: v for k, v in os.environ.items()
           if k not in VARIANT_FLAGS and k != "RELORA_AMD_DISABLE_OPS"}
    env.update(flags)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    t0 = time.monotonic()
    try:
        res = subprocess.run([sys.executable, WORKER, *extra], env=env, cwd=REPO,
                             stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True,
                             timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as ex:
        out = ex.stdout or ""
        _lost(name, f"timeout after {CHILD_TIMEOUT_S:.0f}s",
              out if isinstance(out, str) else out.decode(errors="replace"))
    print(f"gqa variant {name}: child wall time {time.monotonic() - t0:.1f}s")
    if res.returncode != 0:
        _lost(name, f"exit status {res.returncode}", res.stdout)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("ATTN_GQA_RESULT ")]
    if len(lines) != 1:
        _lost(name, "no result line", res.stdout)
    result = json.loads(lines[0].split(" ", 1)[1])
    assert len(result) == (2 if extra else 1), sorted(result)
    print(f"gqa variant {name} err/bound: {result}")
    bad = {c: gc.failures(r) for c, r in result.items() if gc.failures(r)}
    assert not bad, f"{name} {flags}: {bad}"


# (e) group LoRA with unequal sibling widths (q wider than k, v) -------------

def test_lora_group_unequal_siblings(monkeypatch):
    from relora_amd import ops
    from relora_amd.ops import functional as Fn
    from relora_amd.relora import ReLoRaLinear, lora_group_forward

    K, Ns, r, p, M = 256, (256, 128, 128), 32, 0.1, 192
    torch.manual_seed(31)
    mods = []
    for N in Ns:
        m = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=p, bias=False)
        with torch.no_grad():
            m.weight.normal_(std=0.05)
            m.lora_A.weight.normal_(std=0.05)
            m.lora_B.weight.normal_(std=0.05)
        mods.append(m.to(device="cuda", dtype=torch.bfloat16).train())
    g = torch.Generator().manual_seed(32)
    x0 = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    dys = [torch.randn(M, N, generator=g).to(torch.bfloat16).cuda() for N in Ns]

    entered = []
    real = ops.lora_linear_group
    monkeypatch.setattr(ops, "lora_linear_group",
                        lambda *a, **kw: (entered.append(1), real(*a, **kw))[1])

    def one(grouped):
        for m in mods:
            m.zero_grad(set_to_none=True)
        x = x0.detach().clone().requires_grad_(True)
        Fn.set_dropout_rng_state(70)
        ys = lora_group_forward(x, mods) if grouped else [m(x) for m in mods]
        torch.autograd.backward(list(ys), dys)
        return ([y.detach() for y in ys], x.grad,
                [m.lora_A.weight.grad.clone() for m in mods],
                [m.lora_B.weight.grad.clone() for m in mods])

    want = one(False)
    assert not entered
    got = one(True)
    assert len(entered) == 1, "q/k/v with unequal N did not run as one group"

    def close(a, b, tol, name):
        err = (a.double() - b.double()).abs().max().item()
        print(f"lora group unequal {name}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (name, err, tol)

    for i in range(3):
        assert got[0][i].shape == (M, Ns[i])
        close(got[0][i], want[0][i], 0.05 * max(1.0, want[0][i].abs().max().item()), f"y[{i}]")
        close(got[2][i], want[2][i], 0.03 * want[2][i].abs().max().item() + 0.05, f"dA[{i}]")
        close(got[3][i], want[3][i], 0.03 * want[3][i].abs().max().item() + 0.05, f"dB[{i}]")
    close(got[1], want[1], 0.05 * max(1.0, want[1].abs().max().item()), "dx")

    # masks: the group op's per-sibling masks equal the per-module kernel's
    e = ext()
    Fn.set_dropout_rng_state(70)
    seeds = [Fn._next_dropout_seed() & 0x7FFFFFFFFFFFFFFF for _ in mods]
    empty = x0.new_empty(0)
    out = e.lora_group_fwd(
        x0, [m.weight for m in mods], [empty] * 3,
        [m.lora_A.weight.contiguous() for m in mods],
        [m.lora_B.weight.contiguous() for m in mods],
        [float(m._post_lora_scale()) for m in mods], seeds, p,
        [int(Fn._use_fused_k1(x0, m.weight, m.lora_A.weight)) for m in mods])
    masks = out[9:]
    assert len(masks) == 3
    for i, seed in enumerate(seeds):
        _, ref_mask = e.dropout_mask_fwd(x0, p, seed)
        assert torch.equal(masks[i], ref_mask), f"mask of sibling {i}"


# (f) model: 2-layer GQA LLaMA, bf16 HIP path vs fp32 CPU --------------------

def test_llama_gqa_matches_cpu(monkeypatch):
    import copy

    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaForCausalLM
    from relora_amd.ops import functional as Fn
    from relora_amd.relora import ReLoRaModel

    cfg = LlamaConfig(vocab_size=128, hidden_size=256, intermediate_size=344,
                      num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=256)
    torch.manual_seed(0)
    model = ReLoRaModel(LlamaForCausalLM(cfg), r=32, lora_alpha=32, lora_dropout=0.0,
                        target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True)
    with torch.no_grad():  # lora_B starts at zero: give dA something to see
        for n, prm in model.named_parameters():
            if "lora_B" in n:
                prm.normal_(std=0.02)
    attn0 = model.wrapped_model.model.layers[0].self_attn
    assert attn0.k_proj.weight.shape == (128, 256)
    x = torch.randint(0, 128, (2, 128), generator=torch.Generator().manual_seed(1))

    cpu = copy.deepcopy(model).float()
    cpu_loss = cpu(input_ids=x, labels=x).loss
    cpu_loss.backward()

    hip_calls, sdpa_calls = [], []
    real_apply = Fn._HipFlashAttention.apply
    monkeypatch.setattr(Fn._HipFlashAttention, "apply",
                        lambda *a: (hip_calls.append(tuple(a[1].shape)), real_apply(*a))[1])
    real_sdpa = Fn.sdpa_torch
    monkeypatch.setattr(Fn, "sdpa_torch",
                        lambda *a, **kw: (sdpa_calls.append(1), real_sdpa(*a, **kw))[1])
    gpu = model.to("cuda", torch.bfloat16)
    gpu_loss = gpu(input_ids=x.cuda(), labels=x.cuda()).loss
    gpu_loss.backward()
    torch.cuda.synchronize()
    assert hip_calls == [(2, 2, 128, 64)] * 2, hip_calls   # k has nkv heads
    assert not sdpa_calls

    print(f"gqa model loss cpu {cpu_loss.item():.5f} gpu {gpu_loss.item():.5f}")
    assert abs(cpu_loss.item() - gpu_loss.item()) < 0.1, (cpu_loss, gpu_loss)
    refs = {n: prm.grad for n, prm in cpu.named_parameters() if prm.grad is not None}
    gots = {n: prm.grad for n, prm in gpu.named_parameters() if prm.grad is not None}
    assert refs.keys() == gots.keys() and refs
    worst = {}
    for n, ref in refs.items():
        got = gots[n].float().cpu()
        assert torch.isfinite(got).all(), n
        err = (got - ref).abs().max().item()
        worst[n] = err / max(ref.abs().max().item(), 1e-30)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"gqa model worst grad err / |ref|max: {top}")
    # bf16 against fp32: the grad bounds of test_gpu_lora_group.py's model
    # comparison — 0.03*|ref|max + 0.05, and 0.05*|ref|max without the floor
    for n, ref in refs.items():
        err = worst[n] * ref.abs().max().item()
        assert err <= 0.03 * ref.abs().max().item() + 0.05, (n, err)
        assert worst[n] <= 0.05, (n, worst[n])


# (g) host checks raise instead of launching ----------------------------------

def test_host_checks_raise():
    e = ext()
    q = torch.randn(2, 4, 80, 64, device="cuda", dtype=torch.bfloat16)
    k3 = torch.randn(2, 3, 80, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="must divide"):
        e.attn_fwd(q, k3, k3.clone(), 0.125)
    k = torch.randn(2, 2, 80, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="share a layout"):
        e.attn_fwd(q, k, gc.to_layout(k, True), 0.125)
    ks = torch.randn(2, 2, 96, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="agree on batch, sequence"):
        e.attn_fwd(q, ks, ks.clone(), 0.125)
    o, lse = e.attn_fwd(q, k, k.clone(), 0.125)
    with pytest.raises(RuntimeError, match="must divide"):
        e.attn_bwd(q, k3, k3.clone(), o, lse, o, 0.125)
    with pytest.raises(RuntimeError, match="agree on batch, sequence"):
        e.attn_bwd(q, ks, ks.clone(), o, lse, o, 0.125)
    # rope: fewer kv heads pass, a different S raises
    cos, sin = (torch.ones(96, 64, device="cuda"), torch.zeros(96, 64, device="cuda"))
    qo, ko = e.rope_fwd(q, k, cos, sin, False)
    assert qo.shape == q.shape and ko.shape == k.shape
    assert torch.equal(qo, q) and torch.equal(ko, k)
    with pytest.raises(RuntimeError, match="agree on batch, sequence"):
        e.rope_fwd(q, ks, cos, sin, False)
    torch.cuda.synchronize()
