"""Intra-document attention masking on the HIP kernels: `attn_fwd`/`attn_bwd`
with `doc_start` (int32 [B, S]; query i attends to kv j iff
doc_start[b, i] <= j <= i), `flash_attention(doc_start=...)` dispatch and the
LLaMA model.

Reference: float64 masked attention on the CPU (docmask_common.ref_doc).
Bounds are the project's: err <= tol + tol*max(1,|ref|) with tol 2e-2 for
out, 3e-2 for dq/dk/dv, and 1e-2 absolute for lse (attn_variant_worker).
tests/test_doc_mask.py checks on the CPU that the bf16-rounded computation
itself stays inside half of these bounds on the same inputs.
"""

import copy
import functools

import pytest
import torch

import attn_variant_worker as aw
import docmask_common as dc
import gqa_common as gc

pytestmark = pytest.mark.gpu


def ext():
    from relora_amd.ops import hip

    e = hip.ext()
    assert e is not None, "HIP extension not built"
    return e


CASES = {c[0]: c[1:] for c in dc.gpu_cases()}


@functools.lru_cache(maxsize=None)
def case(cid):
    """inputs and reference, computed once and shared (never modified)"""
    nkv, S, hd, ds = CASES[cid]
    inp = dc.make_inputs(nkv, S, hd, ds)
    return inp, ds, dc.ref_doc(*inp, ds)


def run(q, k, v, dout, ds):
    got = dc.run_kernels(ext(), q, k, v, dout, ds)
    torch.cuda.synchronize()
    return got


# (a) boundary grid at S=320, short rows at S=80 and S=33 --------------------

@pytest.mark.parametrize("cid", list(CASES))
def test_boundary_grid(cid):
    (q, k, v, dout), ds, ref = case(cid)
    got = run(*(t.cuda() for t in (q, k, v, dout, ds)))
    assert got["o"].shape == q.shape and got["dq"].shape == q.shape
    assert got["dk"].shape == k.shape and got["dv"].shape == v.shape
    r = aw.all_ratios(got, ref)
    print(f"docmask {cid} err/bound: {r}")
    assert not gc.failures(r), r


@pytest.mark.parametrize("nkv", [4, 2])
def test_one_token_documents(nkv):
    """A one-token document sees only itself: out[i] is v[i] bit for bit
    (P = 1 exactly, every other P is 0, l = 1) and lse[i] is the scaled
    self score.  The lse bound is fp32 rounding of a 64-term dot product and
    the log2 round trip: |s| < 64 here, a few 2^-24 relative, far below 1e-3."""
    (q, k, v, dout), ds, ref = case(f"ones5-hd64-nkv{nkv}")
    got = run(*(t.cuda() for t in (q, k, v, dout, ds)))
    o, lse = got["o"].cpu(), got["lse"].cpu().double()
    vx = gc.expand_kv(v, dc.NH)
    s_self = (q.double() * gc.expand_kv(k, dc.NH).double()).sum(-1) * 64 ** -0.5
    for b, rows in enumerate(dc.ONES5_ROWS):
        for i in rows:
            assert int(ds[b, i]) == i
            assert torch.equal(o[b, :, i], vx[b, :, i]), (b, i)
            err = (lse[b, :, i] - s_self[b, :, i]).abs().max().item()
            assert s_self[b, :, i].abs().max() < 64
            assert err <= 1e-3, (b, i, err)


# (b) all-zero doc_start is the plain causal call, bit for bit ---------------

@pytest.mark.parametrize("hd", [64, 32])
def test_zero_doc_start_is_causal(hd):
    q, k, v, dout = (t.cuda() for t in gc.make_inputs(dc.B, dc.NH, dc.NH, 320, hd))
    base = aw.run_kernels(ext(), q, k, v, dout)
    ds = torch.zeros(dc.B, 320, dtype=torch.int32, device="cuda")
    got = run(q, k, v, dout, ds)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(got[n], base[n]), n


# (c) the four q/kv layout pairs ---------------------------------------------

def test_layouts():
    (q, k, v, dout), ds, ref = case("b300-hd64-nkv2")
    base = run(*(t.cuda() for t in (q, k, v, dout, ds)))
    for q_t in (False, True):
        for kv_t in (False, True):
            qq = gc.to_layout(q.cuda(), q_t)
            kk, vv = gc.to_layout(k.cuda(), kv_t), gc.to_layout(v.cuda(), kv_t)
            got = run(qq, kk, vv, dout.cuda(), ds.cuda())
            assert got["dk"].stride() == kk.stride() and got["o"].stride() == qq.stride()
            r = aw.all_ratios(got, ref)
            print(f"docmask layout q_t={q_t} kv_t={kv_t} err/bound: {r}")
            assert not gc.failures(r), (q_t, kv_t, r)
            for n in ("o", "lse", "dq", "dk", "dv"):
                assert torch.equal(got[n], base[n]), (q_t, kv_t, n)


# (d) dispatch: padded hd <= 64 reaches the extension, the rest masked SDPA --

def _flash_with_spies(hd, monkeypatch):
    from relora_amd.ops import functional as Fn

    S = 160
    ds = dc.doc_start_from_lengths(([45, 115], [160]), S)
    q, k, v, dout = dc.make_inputs(2, S, hd, ds, seed=3)
    ref = dc.ref_doc(q, k, v, dout, ds)
    hip_calls, sdpa_calls = [], []
    real_apply = Fn._HipFlashAttention.apply
    monkeypatch.setattr(
        Fn._HipFlashAttention, "apply",
        lambda *a: (hip_calls.append(len(a) == 5 and a[4] is not None), real_apply(*a))[1])
    real_sdpa = Fn.sdpa_torch
    monkeypatch.setattr(
        Fn, "sdpa_torch",
        lambda *a, **kw: (sdpa_calls.append(kw.get("doc_start") is not None),
                          real_sdpa(*a, **kw))[1])
    qg, kg, vg = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = Fn.flash_attention(qg, kg, vg, doc_start=ds.cuda())
    o.backward(dout.cuda())
    torch.cuda.synchronize()
    got = {"o": o.detach(), "dq": qg.grad, "dk": kg.grad, "dv": vg.grad}
    r = {"o": aw.bound_ratio(got["o"], ref["o"], aw.FWD_TOL), **aw.grad_ratios(got, ref)}
    print(f"docmask dispatch hd{hd} err/bound: {r}")
    return hip_calls, sdpa_calls, r


@pytest.mark.parametrize("hd", [64, 48, 32])
def test_dispatch_reaches_extension(hd, monkeypatch):
    hip_calls, sdpa_calls, r = _flash_with_spies(hd, monkeypatch)
    assert hip_calls == [True] and not sdpa_calls
    assert not gc.failures(r), r


@pytest.mark.parametrize("hd", [128, 80, 52])
def test_dispatch_takes_masked_sdpa(hd, monkeypatch):
    hip_calls, sdpa_calls, r = _flash_with_spies(hd, monkeypatch)
    assert sdpa_calls == [True] and not hip_calls
    assert not gc.failures(r), r


def test_host_checks_raise():
    e = ext()
    q = torch.randn(2, 4, 80, 64, device="cuda", dtype=torch.bfloat16)
    ds = torch.zeros(2, 80, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="int32"):
        e.attn_fwd(q, q, q, 0.125, ds.long())
    with pytest.raises(RuntimeError, match=r"\[B, S\]"):
        e.attn_fwd(q, q, q, 0.125, ds[:, :40].contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        e.attn_fwd(q, q, q, 0.125, torch.zeros(80, 2, dtype=torch.int32, device="cuda").t())
    with pytest.raises(RuntimeError, match="q's device"):
        e.attn_fwd(q, q, q, 0.125, ds.cpu())
    q128 = torch.randn(2, 4, 80, 128, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="head_dim <= 64"):
        e.attn_fwd(q128, q128, q128, 0.125, ds)
    o, lse = e.attn_fwd(q, q, q, 0.125, ds)
    with pytest.raises(RuntimeError, match="int32"):
        e.attn_bwd(q, q, q, o, lse, o, 0.125, ds.long())
    torch.cuda.synchronize()


# (e) model: 2-layer LLaMA, bf16 HIP path with doc_start vs fp32 CPU ---------

@pytest.mark.parametrize("variant", ["gqa", "checkpointing"])
def test_llama_doc_start_matches_cpu(variant, monkeypatch):
    from relora_amd import ops
    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaForCausalLM
    from relora_amd.ops import functional as Fn

    cfg = LlamaConfig(vocab_size=128, hidden_size=256, intermediate_size=344,
                      num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2 if variant == "gqa" else 4,
                      max_position_embeddings=256)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).train()
    model.model.gradient_checkpointing = variant == "checkpointing"
    x = torch.randint(2, 128, (2, 128), generator=torch.Generator().manual_seed(1))
    x[0, [40, 41, 99]] = 1          # eos = 1: documents end at these tokens
    x[1, [63]] = 1
    ds = ops.doc_starts_from_eos(x, 1)
    assert dc.is_well_formed(ds) and ds.max() == 100

    cpu = copy.deepcopy(model).float()
    cpu_loss = cpu(input_ids=x, labels=x, doc_start=ds).loss
    cpu_loss.backward()

    hip_calls, sdpa_calls = [], []
    real_apply = Fn._HipFlashAttention.apply
    monkeypatch.setattr(
        Fn._HipFlashAttention, "apply",
        lambda *a: (hip_calls.append(len(a) == 5 and a[4] is not None), real_apply(*a))[1])
    real_sdpa = Fn.sdpa_torch
    monkeypatch.setattr(Fn, "sdpa_torch",
                        lambda *a, **kw: (sdpa_calls.append(1), real_sdpa(*a, **kw))[1])
    gpu = model.to("cuda", torch.bfloat16)
    gpu_loss = gpu(input_ids=x.cuda(), labels=x.cuda(), doc_start=ds.cuda()).loss
    gpu_loss.backward()
    torch.cuda.synchronize()
    # checkpointing runs every layer's forward a second time
    assert hip_calls == [True] * (4 if variant == "checkpointing" else 2), hip_calls
    assert not sdpa_calls

    print(f"docmask model {variant} loss cpu {cpu_loss.item():.5f} gpu {gpu_loss.item():.5f}")
    assert abs(cpu_loss.item() - gpu_loss.item()) < 0.1, (cpu_loss, gpu_loss)
    refs = {n: prm.grad for n, prm in cpu.named_parameters() if prm.grad is not None}
    gots = {n: prm.grad for n, prm in gpu.named_parameters() if prm.grad is not None}
    assert refs.keys() == gots.keys() and refs
    worst = {}
    for n, ref in refs.items():
        got = gots[n].float().cpu()
        assert torch.isfinite(got).all(), n
        worst[n] = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"docmask model {variant} worst grad err / |ref|max: {top}")
    # the bounds of test_gpu_attention_gqa.py::test_llama_gqa_matches_cpu
    for n, ref in refs.items():
        err = worst[n] * ref.abs().max().item()
        assert err <= 0.03 * ref.abs().max().item() + 0.05, (n, err)
        assert worst[n] <= 0.05, (n, worst[n])
