"""Attention edge tests: the v3 forward's rescale / defer-max branches with
non-zero accumulators, numerics of the strided (transposed-BSHD) layout the
models use, tile-boundary sequence lengths, the environment-selected kernel
variants (one fresh child process each), and the SDPA dispatch guard.

Reference everywhere: plain float64 causal softmax attention on the CPU with
its autograd backward, from the bf16 inputs upcast.  Bounds are the
project's (assert_close_bf16): err <= tol + tol*max(1,|ref|) with tol 2e-2
for the forward and 3e-2 for gradients, and 1e-2 absolute for lse.

Helpers live in attn_variant_worker.py (same directory), which is also the
child-process entry point for the variant tests.
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

gpu = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "attn_variant_worker.py")
HDS = (64, 128, 32)


def ext():
    from relora_amd.ops import hip

    e = hip.ext()
    assert e is not None, "HIP extension not built"
    return e


def cuda(*ts):
    out = tuple(t.cuda() for t in ts)
    for a, b in zip(ts, out):
        assert a.stride() == b.stride()
    return out


@functools.lru_cache(maxsize=None)
def structured(kind, hd):
    """inputs + float64 reference of one structured set, computed once and
    shared (read-only) by the CPU, forward and backward tests."""
    q, k, v, dout = aw.make_structured(kind, hd)
    return (q, k, v, dout), aw.ref_attention(q, k, v, dout)


def failures(ratios, limit=1.0):
    """names whose bound ratio exceeds `limit` (lse: absolute, vs LSE_TOL)."""
    bad = {}
    for name, r in ratios.items():
        lim = aw.LSE_TOL if name.endswith("lse") else limit
        if not r <= lim:
            bad[name] = r
    return bad


# ---------------------------------------------------------------------------
# A. rescale / deferred-max / descending inputs
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("kind", aw.STRUCTURED_KINDS)
def test_structured_inputs_cpu(kind, hd):
    """No GPU: the inputs hit the branch they are built for (replayed on the
    float64 log2-domain scores), and a bf16-emulated float64 result meets
    every bound with at least 2x headroom — so a kernel failure on these
    inputs is the kernel's, not the inputs'."""
    (q, k, v, dout), ref = structured(kind, hd)
    stats = aw.check_structured_conditions(kind, q, k)
    emu = aw.all_ratios(aw.emulate_bf16(q, k, v, dout), ref)
    print(f"{kind} hd{hd}: {stats} emulation/bound {emu}")
    lse_err = emu.pop("lse")
    assert lse_err <= aw.LSE_TOL / 2, lse_err
    assert not failures(emu, limit=0.5), emu


@gpu
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("kind", aw.STRUCTURED_KINDS)
def test_structured_fwd(kind, hd):
    (q, k, v, dout), ref = structured(kind, hd)
    aw.check_structured_conditions(kind, q, k)   # before any kernel runs
    qg, kg, vg = cuda(q, k, v)
    o, lse = ext().attn_fwd(qg, kg, vg, hd ** -0.5)
    hot = aw.hot_row_mask(q.shape[-2])
    o = o.cpu()
    r = {
        "hot rows o": aw.bound_ratio(o[..., hot, :], ref["o"][..., hot, :], aw.FWD_TOL),
        "cold rows o": aw.bound_ratio(o[..., ~hot, :], ref["o"][..., ~hot, :], aw.FWD_TOL),
        "hot rows lse": float((lse.cpu().double() - ref["lse"])[..., hot].abs().max()),
        "cold rows lse": float((lse.cpu().double() - ref["lse"])[..., ~hot].abs().max()),
    }
    print(f"{kind} hd{hd} fwd err/bound: {r}")
    assert not failures(r), f"{kind} hd{hd}: {failures(r)} (all: {r})"


@gpu
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("kind", aw.STRUCTURED_KINDS)
def test_structured_bwd(kind, hd):
    (q, k, v, dout), ref = structured(kind, hd)
    aw.check_structured_conditions(kind, q, k)
    got = aw.run_kernels(ext(), *cuda(q, k, v, dout))
    hot = aw.hot_row_mask(q.shape[-2])
    r = aw.grad_ratios(got, ref)
    r["hot rows dq"] = aw.bound_ratio(got["dq"][..., hot, :], ref["dq"][..., hot, :],
                                      aw.GRAD_TOL)
    r["cold rows dq"] = aw.bound_ratio(got["dq"][..., ~hot, :], ref["dq"][..., ~hot, :],
                                       aw.GRAD_TOL)
    print(f"{kind} hd{hd} bwd err/bound: {r}")
    assert not failures(r), f"{kind} hd{hd}: {failures(r)} (all: {r})"


# ---------------------------------------------------------------------------
# B. strided (transposed-BSHD) layout numerics
# ---------------------------------------------------------------------------


def assert_same(a, b, what):
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[n], b[n]), (
            f"{what}: {n} differs, max {(a[n].float() - b[n].float()).abs().max().item()}")


@gpu
@pytest.mark.parametrize("hd", (64, 128))
def test_strided_layout_numerics(hd):
    """The kernels have no atomics and a layout only changes addresses, so
    strided and contiguous runs must agree bit for bit — whichever layout
    dout arrives in — and both must match float64."""
    B, nh, S = 2, 3, 160
    q, k, v, dout = cuda(*aw.strided_qkv(B, nh, S, hd, n=4))
    assert q.stride() == (S * nh * hd, hd, nh * hd, 1) and not q.is_contiguous()
    ref = aw.ref_attention(q, k, v, dout)
    e = ext()

    strided = aw.run_kernels(e, q, k, v, dout)
    assert strided["o"].stride() == q.stride() and strided["dq"].stride() == q.stride()
    r = aw.all_ratios(strided, ref)
    print(f"strided hd{hd} err/bound: {r}")
    assert not failures(r), r

    qc, kc, vc, dc = (t.contiguous() for t in (q, k, v, dout))
    contig = aw.run_kernels(e, qc, kc, vc, dc)
    assert_same(strided, contig, "strided vs contiguous")
    # dout in the other layout: attn_bwd re-lays it out to q's
    assert_same(aw.run_kernels(e, q, k, v, dc), strided, "contiguous dout, strided q")
    assert_same(aw.run_kernels(e, qc, kc, vc, dout), strided, "strided dout, contiguous q")

    # stride-0 dout, as out.sum().backward() hands over
    ones = torch.ones((), device="cuda", dtype=torch.bfloat16).expand(B, nh, S, hd)
    assert ones.stride() == (0, 0, 0, 0)
    exp_s = aw.run_kernels(e, q, k, v, ones)
    assert_same(exp_s, aw.run_kernels(e, qc, kc, vc, ones), "expanded dout")
    r = aw.all_ratios(exp_s, aw.ref_attention(q, k, v, ones))
    print(f"strided hd{hd} expanded-dout err/bound: {r}")
    assert not failures(r), r


@gpu
@pytest.mark.parametrize("hd", (64, 128))
def test_strided_autograd_values(hd):
    """fops.flash_attention on the models' layout: gradient values against
    float64, for an ordinary dout and for the expanded one of .sum()."""
    from relora_amd import ops as fops

    B, nh, S = 2, 3, 160
    g = torch.Generator().manual_seed(7)
    bufs = [torch.randn(B, S, nh * hd, generator=g).to(torch.bfloat16).cuda().requires_grad_()
            for _ in range(3)]
    dout = torch.randn(B, nh, S, hd, generator=g).to(torch.bfloat16).cuda()
    q, k, v = (b.view(B, S, nh, hd).transpose(1, 2) for b in bufs)

    def bshd(t):  # reference grads [B,nh,S,hd] -> the leaf buffers' layout
        return t.transpose(1, 2).reshape(B, S, nh * hd)

    for what, d in (("dout", dout), ("sum", None)):
        for b in bufs:
            b.grad = None
        out = fops.flash_attention(q, k, v, causal=True)
        assert out.stride() == q.stride()
        if d is None:
            out.sum().backward()
            d = torch.ones_like(dout)
        else:
            out.backward(d)
        ref = aw.ref_attention(q, k, v, d)
        r = {"o": aw.bound_ratio(out, ref["o"], aw.FWD_TOL)}
        for n, b in zip(("dq", "dk", "dv"), bufs):
            r[n] = aw.bound_ratio(b.grad, bshd(ref[n]), aw.GRAD_TOL)
        print(f"autograd hd{hd} {what} err/bound: {r}")
        assert not failures(r), f"{what}: {r}"


# ---------------------------------------------------------------------------
# C. tile-edge sweep
# ---------------------------------------------------------------------------

EDGE_S = (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 255, 256, 257, 321)


def sweep(hd, lengths):
    """fwd+bwd at B=1, nh=2 (odd S then misaligns the second head's
    lse/delta quads); returns {S: failing ratios}."""
    e = ext()
    bad = {}
    for S in lengths:
        g = torch.Generator().manual_seed(100 * hd + S)
        q, k, v, dout = (torch.randn(1, 2, S, hd, generator=g).to(torch.bfloat16)
                         for _ in range(4))
        ref = aw.ref_attention(q, k, v, dout)
        r = aw.all_ratios(aw.run_kernels(e, *cuda(q, k, v, dout)), ref)
        print(f"S={S} hd={hd} err/bound: {r}")
        if failures(r):
            bad[S] = failures(r)
    return bad


@gpu
@pytest.mark.parametrize("hd", (32, 64, 128))
def test_tile_edges(hd):
    bad = sweep(hd, EDGE_S)
    assert not bad, f"hd={hd}: {bad}"


@gpu
@pytest.mark.parametrize("hd", (40, 72, 104))
def test_tile_edges_padded_hd(hd):
    """head dims that are zero-padded up to the 64/96/128 templates"""
    bad = sweep(hd, (33, 257))
    assert not bad, f"hd={hd}: {bad}"


# ---------------------------------------------------------------------------
# D. environment-selected variants, one fresh child process each
# ---------------------------------------------------------------------------

VARIANT_FLAGS = ("RELORA_AMD_ATTN_FWD", "RELORA_AMD_ATTN_BWD", "RELORA_AMD_ATTN_OCC4",
                 "RELORA_AMD_ATTN_TR_FWD", "RELORA_AMD_ATTN_TR_DKDV",
                 "RELORA_AMD_DQ_4WAVE", "RELORA_AMD_DQ_OCC4")
VARIANTS = {
    "v2_fwd_bwd": ({"RELORA_AMD_ATTN_FWD": "2", "RELORA_AMD_ATTN_BWD": "2"}, ["--hd128"]),
    "fwd_occ4_off": ({"RELORA_AMD_ATTN_OCC4": "0"}, []),
    "tr_fwd_off_tr_dkdv_dq4wave": ({"RELORA_AMD_ATTN_TR_FWD": "0",
                                    "RELORA_AMD_ATTN_TR_DKDV": "1",
                                    "RELORA_AMD_DQ_4WAVE": "1"}, []),
    "dq_occ4": ({"RELORA_AMD_DQ_OCC4": "1"}, []),
}
# Measured on MI355X hosts: 2.8 - 3.0 s wall time per child in one run,
# 3.1 - 3.9 s (mean 3.5) in another (interpreter start, torch import and GPU
# init dominate; the kernels are milliseconds).  The limit is 5x the larger
# mean.
CHILD_WALL_S = 3.5
CHILD_TIMEOUT_S = 5 * CHILD_WALL_S

# Name of the first child that ended by signal, abort, timeout or any other
# way without a result.  Once set, no further child is launched: whatever
# took it down must be understood from the kernel code first.
_casualty = None


def _lost(name, how, tail=""):
    global _casualty
    _casualty = f"{name} ({how})"
    pytest.fail(f"variant child {_casualty}; output tail:\n{tail[-2000:]}")


@gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_child(name):
    if _casualty is not None:
        pytest.fail(f"not launched: variant child {_casualty} went down first")
    try:  # a GPU error left behind by an earlier test also bars new processes
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
    print(f"variant {name}: child wall time {time.monotonic() - t0:.1f}s")
    if res.returncode != 0:
        _lost(name, f"exit status {res.returncode}", res.stdout)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("ATTN_VARIANT_RESULT ")]
    if len(lines) != 1:
        _lost(name, "no result line", res.stdout)
    result = json.loads(lines[0].split(" ", 1)[1])
    expected = 2 + 2 * (3 if extra else 2) + (1 if extra else 0)
    assert len(result) == expected, sorted(result)
    bad = {case: failures(r) for case, r in result.items() if failures(r)}
    print(f"variant {name} err/bound: {result}")
    assert not bad, f"{name} {flags}: {bad}"


# ---------------------------------------------------------------------------
# E. dispatch guard: what the kernels don't take goes to SDPA
# ---------------------------------------------------------------------------


def _run_flash(dtype, hd, S=80):
    from relora_amd import ops as fops

    g = torch.Generator().manual_seed(hd)
    q, k, v, dout = (torch.randn(1, 2, S, hd, generator=g).to(dtype).cuda()
                     for _ in range(4))
    for t in (q, k, v):
        t.requires_grad_()
    out = fops.flash_attention(q, k, v, causal=True)
    out.backward(dout)
    ref = aw.ref_attention(q, k, v, dout)
    r = {"o": aw.bound_ratio(out, ref["o"], aw.FWD_TOL)}
    r.update(aw.grad_ratios({"dq": q.grad, "dk": k.grad, "dv": v.grad}, ref))
    return r


def shipped_head_dims():
    """{head_dim: [config names]} over configs/*.json"""
    import glob

    dims = {}
    for path in sorted(glob.glob(os.path.join(REPO, "configs", "*.json"))):
        with open(path) as f:
            cfg = json.load(f)
        hd = cfg["hidden_size"] // cfg["num_attention_heads"]
        dims.setdefault(hd, []).append(os.path.basename(path)[:-len(".json")])
    return dims


# hd of the shipped configs that the kernels take / that the guard gives to
# SDPA.  52 is llama_40m (416 / 8 heads): not a multiple of 8, so its rows
# are not 16-byte aligned.  It ran on the HIP kernels before the guard,
# with no numerics test; routing it to SDPA is a decision, pinned here.
HIP_HDS = (32, 48, 64, 80, 128)
SDPA_HDS = (52,)


def test_shipped_head_dims_are_pinned():
    """No GPU: every head dim of configs/*.json is on one of the two lists
    the dispatch tests run, and only llama_40m is on SDPA's."""
    dims = shipped_head_dims()
    assert set(dims) == set(HIP_HDS) | set(SDPA_HDS), dims
    assert {hd: dims[hd] for hd in SDPA_HDS} == {52: ["llama_40m"]}


@gpu
@pytest.mark.parametrize("dtype,hd", [(torch.float32, 64), (torch.bfloat16, 256),
                                      (torch.bfloat16, 36)]
                         + [(torch.bfloat16, hd) for hd in SDPA_HDS])
def test_dispatch_guard_uses_sdpa(dtype, hd, monkeypatch):
    """float32, hd > 128 and hd % 8 != 0 never reach the HIP kernels; the
    last includes llama_40m's hd=52."""
    from relora_amd.ops import functional

    def no_hip(*a, **kw):
        raise AssertionError("reached the HIP attention kernels")

    monkeypatch.setattr(functional._HipFlashAttention, "apply", no_hip)
    r = _run_flash(dtype, hd)
    print(f"guard {dtype} hd{hd} err/bound: {r}")
    assert not failures(r), r


@gpu
@pytest.mark.parametrize("hd", HIP_HDS)
def test_dispatch_keeps_hip_path(hd, monkeypatch):
    """every head dim of the shipped configs that is a multiple of 8 (all
    but llama_40m's 52) still runs the HIP kernels, through autograd; 80
    (llama_3b) uses the zero-padded 96 template"""
    from relora_amd.ops import functional

    calls = []
    real = functional._HipFlashAttention.apply

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(functional._HipFlashAttention, "apply", spy)
    r = _run_flash(torch.bfloat16, hd)
    assert calls == [1]
    assert not failures(r), r
