"""The per-head QK RMSNorm + RoPE kernels (ops/csrc/qk_norm_rope.hip) against
a float64 CPU reference of the unrounded chain rope(w * x * invrms) and its
analytic gradients (tests/qk_norm_common.py): a value grid over every head
dim and head grouping, all layout pairs, exact values, the row coverage of
the deterministic dw reduction, determinism, host-check rejections and the
dispatch of ops.qk_norm_rope."""

import os
import subprocess
import sys

import pytest
import torch

import qk_norm_common as qc
from relora_amd import ops
from relora_amd.ops import functional as Fn
from relora_amd.ops import hip

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-5


def _tables(hd, rows=96):
    cos, sin = ops.build_rope_cache(hd, rows)
    return cos.cuda(), sin.cuda()


def _run_kernels(xq, xk, wq, wk, dyq, dyk, cos, sin, eps, lq="bshd", lk="bshd"):
    """forward + backward through the extension entries: fp32 dw, no autograd"""
    ext = hip.ext()
    q, k = qc.in_layout(xq.cuda(), lq), qc.in_layout(xk.cuda(), lk)
    dq_in, dk_in = qc.in_layout(dyq.cuda(), lq), qc.in_layout(dyk.cuda(), lk)
    wq, wk = wq.cuda(), wk.cuda()
    qo, ko, iq, ik = ext.qk_norm_rope_fwd(q, k, wq, wk, cos, sin, eps)
    assert qo.stride() == q.stride() and ko.stride() == k.stride()
    assert iq.shape == q.shape[:3] and iq.is_contiguous() and iq.dtype == torch.float32
    assert ik.shape == k.shape[:3] and ik.is_contiguous()
    dq, dk, dwq, dwk = ext.qk_norm_rope_bwd(dq_in, dk_in, q, k, wq, wk, iq, ik, cos, sin)
    assert dq.stride() == q.stride() and dk.stride() == k.stride()
    assert dwq.dtype == torch.float32 and dwq.shape == wq.shape and dwk.shape == wk.shape
    torch.cuda.synchronize()
    return qo, ko, iq, ik, dq, dk, dwq, dwk


# -- 1. value grid ---------------------------------------------------------------

@pytest.mark.parametrize("S", [80, 33])
@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("hd", [32, 48, 64, 80, 128])
def test_value_grid(hd, nh, nkv, S):
    """Element bounds, one 2^-8 term per bf16 intermediate:
    out  3 * 2^-8 * (|y1 cos| + |y2 sin|) + hd * 2^-23 * (same)
    dx   2^-8 * |dx| + hd * 2^-23 * invrms * (|dn| + |nhat| mean|dn nhat|)
    dw   rows * 2^-23 * sum_rows |g nhat|       invrms  relative 2^-21
    The worst observed fractions of the bounds are in
    profiles/stage13_qk_norm.md."""
    B = 2
    xq, wq, dyq = qc.make_case(B, nh, S, hd, seed=hd * 1000 + S)
    xk, wk, dyk = qc.make_case(B, nkv, S, hd, seed=hd * 1000 + S + 500 + nkv)
    cos, sin = _tables(hd)
    got = _run_kernels(xq, xk, wq, wk, dyq, dyk, cos, sin, EPS)
    qo, ko, iq, ik, dq, dk, dwq, dwk = got
    worst = {}
    for name, x, w, dy, o, ir, dx, dw in (("q", xq, wq, dyq, qo, iq, dq, dwq),
                                          ("k", xk, wk, dyk, ko, ik, dk, dwk)):
        ref = qc.reference(x, w, dy, cos.cpu(), sin.cpu(), EPS)
        worst[name + "_out"] = qc.worst_fraction(o, ref["out"], ref["out_bound"])
        worst[name + "_dx"] = qc.worst_fraction(dx, ref["dx"], ref["dx_bound"])
        worst[name + "_dw"] = qc.worst_fraction(dw, ref["dw"], ref["dw_bound"])
        worst[name + "_invrms"] = qc.worst_fraction(
            ir, ref["invrms"], 2.0 ** -21 * ref["invrms"])
        # the all-zero row: output 0, finite gradients
        b, h, s = x.shape[0] - 1, x.shape[1] - 1, S // 2
        assert not x[b, h, s].any()
        assert torch.equal(o[b, h, s].cpu(), torch.zeros(hd, dtype=torch.bfloat16))
        assert torch.isfinite(dx.float()).all() and torch.isfinite(dw).all()
        assert torch.isfinite(o.float()).all() and torch.isfinite(ir).all()
    print(f"QKN_FRAC hd{hd} nh{nh} nkv{nkv} S{S} "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


# -- 2. layouts -------------------------------------------------------------------

@pytest.mark.parametrize("hd", [48, 128])
def test_layout_pairs_bit_equal(hd):
    B, nh, nkv, S = 2, 4, 2, 33
    xq, wq, dyq = qc.make_case(B, nh, S, hd, seed=1)
    xk, wk, dyk = qc.make_case(B, nkv, S, hd, seed=2)
    cos, sin = _tables(hd)
    base = None
    for lq in ("bhsd", "bshd"):
        for lk in ("bhsd", "bshd"):
            got = _run_kernels(xq, xk, wq, wk, dyq, dyk, cos, sin, EPS, lq, lk)
            if base is None:
                base = got
                continue
            for a, b in zip(base, got):
                assert torch.equal(a, b), (lq, lk)
    # through autograd, dout given in the other layout than q / k
    other = {"bhsd": "bshd", "bshd": "bhsd"}
    for lq, lk in (("bhsd", "bshd"), ("bshd", "bhsd")):
        q = qc.in_layout(xq.cuda(), lq).detach().requires_grad_()
        k = qc.in_layout(xk.cuda(), lk).detach().requires_grad_()
        wq_, wk_ = wq.cuda().requires_grad_(), wk.cuda().requires_grad_()
        qo, ko = ops.qk_norm_rope(q, k, wq_, wk_, cos, sin, EPS)
        douts = (qc.in_layout(dyq.cuda(), other[lq]), qc.in_layout(dyk.cuda(), other[lk]))
        assert douts[0].stride() != q.stride() and douts[1].stride() != k.stride()
        dq, dk, dwq, dwk = torch.autograd.grad((qo, ko), (q, k, wq_, wk_), douts)
        assert torch.equal(qo, base[0]) and torch.equal(ko, base[1])
        assert torch.equal(dq, base[4]) and torch.equal(dk, base[5])
        assert torch.equal(dwq, base[6].to(torch.bfloat16))
        assert torch.equal(dwk, base[7].to(torch.bfloat16))


# -- 3. exact values ----------------------------------------------------------------

@pytest.mark.parametrize("hd", [32, 48, 64, 80, 128])
def test_exact_values(hd):
    """eps = 0, rows of +-2^k entries (one k per row), power-of-two weights,
    (cos, sin) from {(1,0), (0,1), (-1,0), (0,-1)} by position: every
    intermediate is exactly representable, so the outputs equal the float64
    reference bit for bit, whole buffers compared."""
    B, nh, nkv, S = 2, 4, 2, 37
    g = torch.Generator().manual_seed(hd)

    def rows(heads):
        sign = torch.randint(0, 2, (B, heads, S, hd), generator=g).float() * 2 - 1
        k = torch.randint(-6, 7, (B, heads, S, 1), generator=g).float()
        return (sign * 2.0 ** k).to(torch.bfloat16)

    def weight():
        sign = torch.randint(0, 2, (hd,), generator=g).float() * 2 - 1
        return (sign * 2.0 ** torch.randint(-2, 3, (hd,), generator=g).float()).to(
            torch.bfloat16)

    xq, xk, wq, wk = rows(nh), rows(nkv), weight(), weight()
    pos = torch.arange(S + 3) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[pos][:, None].expand(-1, hd).contiguous()
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[pos][:, None].expand(-1, hd).contiguous()
    ext = hip.ext()
    for lq, lk in (("bshd", "bshd"), ("bhsd", "bshd")):
        q, k = qc.in_layout(xq.cuda(), lq), qc.in_layout(xk.cuda(), lk)
        qo, ko, iq, ik = ext.qk_norm_rope_fwd(q, k, wq.cuda(), wk.cuda(), cos.cuda(),
                                              sin.cuda(), 0.0)
        for o, x, w in ((qo, xq, wq), (ko, xk, wk)):
            ref = qc.reference(x, w, torch.zeros_like(x), cos, sin, 0.0)["out"]
            assert torch.equal(ref.to(torch.bfloat16).double(), ref)   # representable
            assert torch.equal(o.cpu().double(), ref)


# -- 4. row coverage of the dw reduction ----------------------------------------------

def _coverage_shapes(hd):
    rpb, cap = hip.ext().qk_norm_rope_geometry(hd)
    B, nh, nkv = 2, 8, 4
    # q strides more than twice over the capped grid, k (half the rows) more than once
    S_big = (2 * cap * rpb) // (B * nh) + 4
    assert B * nh * S_big > 2 * cap * rpb and B * nkv * S_big > cap * rpb
    assert B * nh * S_big < 2 ** 22
    return {
        "below_one_block": (1, 2, 1, 7),
        "ragged": (1, 4, 2, rpb // 2 + 5),      # q: 2 * rpb + 20 rows, k: rpb + 10
        "strided": (B, nh, nkv, S_big),
    }


@pytest.mark.parametrize("which", ["below_one_block", "ragged", "strided"])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_dw_row_coverage(hd, which):
    """x = +-1, eps = 0, identity tables, dy = sign(x): every row adds exactly
    1 to every dw_j, so one dropped or doubled row is outside rows * 2^-22."""
    B, nh, nkv, S = _coverage_shapes(hd)[which]
    rpb, cap = hip.ext().qk_norm_rope_geometry(hd)
    g = torch.Generator().manual_seed(S)
    ext = hip.ext()
    xq = (torch.randint(0, 2, (B, nh, S, hd), generator=g).float() * 2 - 1).to(torch.bfloat16)
    xk = (torch.randint(0, 2, (B, nkv, S, hd), generator=g).float() * 2 - 1).to(torch.bfloat16)
    rows_q, rows_k = B * nh * S, B * nkv * S
    assert rows_q != rows_k
    if which == "below_one_block":
        assert rows_q < rpb
    if which == "ragged":
        assert rows_q % rpb and rows_k % rpb and rows_q > rpb
    q = qc.in_layout(xq.cuda(), "bshd")
    k = qc.in_layout(xk.cuda(), "bhsd")
    w = torch.ones(hd, dtype=torch.bfloat16, device="cuda")
    cos = torch.ones(S, hd, device="cuda")
    sin = torch.zeros(S, hd, device="cuda")
    qo, ko, iq, ik = ext.qk_norm_rope_fwd(q, k, w, w, cos, sin, 0.0)
    assert torch.equal(qo, q) and torch.equal(ko, k)
    assert torch.equal(iq, torch.ones_like(iq)) and torch.equal(ik, torch.ones_like(ik))
    dq, dk, dwq, dwk = ext.qk_norm_rope_bwd(q, k, q, k, w, w, iq, ik, cos, sin)
    torch.cuda.synchronize()
    for dw, rows in ((dwq, rows_q), (dwk, rows_k)):
        err = (dw.double().cpu() - rows).abs().max().item()
        print(f"QKN_ROWS hd{hd} {which} rows {rows} max|dw - rows| {err}")
        assert err <= rows * 2.0 ** -22, (rows, err)
    # dn = nhat here, so dx = invrms * (dn - nhat * 1) = 0
    assert not dq.any() and not dk.any()


# -- 5. determinism ---------------------------------------------------------------------

def test_two_calls_bit_equal():
    hd, B, nh, nkv = 64, 2, 8, 2
    rpb, cap = hip.ext().qk_norm_rope_geometry(hd)
    S = cap * rpb // (B * nh) + 9          # q's blocks stride
    xq, wq, dyq = qc.make_case(B, nh, S, hd, seed=5)
    xk, wk, dyk = qc.make_case(B, nkv, S, hd, seed=6)
    cos, sin = _tables(hd, S)
    a = _run_kernels(xq, xk, wq, wk, dyq, dyk, cos, sin, EPS)
    b = _run_kernels(xq, xk, wq, wk, dyq, dyk, cos, sin, EPS)
    assert len(a) == 8
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# -- 6. rejections ------------------------------------------------------------------------

def _good(hd=64, B=2, nh=4, nkv=2, S=16):
    dev = "cuda"
    q = torch.randn(B, S, nh, hd, device=dev).to(torch.bfloat16).transpose(1, 2)
    k = torch.randn(B, S, nkv, hd, device=dev).to(torch.bfloat16).transpose(1, 2)
    w = torch.ones(hd, dtype=torch.bfloat16, device=dev)
    cos, sin = _tables(hd, S + 4)
    return dict(q=q, k=k, wq=w, wk=w.clone(), cos=cos, sin=sin, eps=1e-6)


def _unaligned(t):
    """the same values 8 bytes off a 16-byte boundary"""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)[4:4 + t.numel()]
    out = flat.view(t.shape) if t.is_contiguous() else \
        flat.view(t.transpose(1, 2).shape).transpose(1, 2)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8
    return out


FWD_REJECTS = {
    "q_fp32": (lambda a: a.update(q=a["q"].float()), "bf16"),
    "k_on_cpu": (lambda a: a.update(k=a["k"].cpu()), "one GPU"),
    "q_layout": (lambda a: a.update(q=a["q"].repeat(1, 1, 2, 1)[:, :, ::2]), "BHSD-contiguous"),
    "k_layout": (lambda a: a.update(k=a["k"].contiguous()[:, :, ::2]), "BHSD-contiguous"),
    "k_other_S": (lambda a: a.update(k=a["k"][:, :, :8].contiguous()), "agree on batch"),
    "k_other_B": (lambda a: a.update(k=a["k"][:1].contiguous()), "agree on batch"),
    "hd_24": (lambda a: a.update(
        q=torch.zeros(1, 1, 4, 24, dtype=torch.bfloat16, device="cuda"),
        k=torch.zeros(1, 1, 4, 24, dtype=torch.bfloat16, device="cuda")), "multiple of 16"),
    "hd_256": (lambda a: a.update(
        q=torch.zeros(1, 1, 4, 256, dtype=torch.bfloat16, device="cuda"),
        k=torch.zeros(1, 1, 4, 256, dtype=torch.bfloat16, device="cuda")), "at most 128"),
    "partial_rotary": (lambda a: a.update(cos=a["cos"][:, :32].contiguous(),
                                          sin=a["sin"][:, :32].contiguous()), "full rotary"),
    "cos_fp64": (lambda a: a.update(cos=a["cos"].double()), "fp32 contiguous tables"),
    "sin_strided": (lambda a: a.update(sin=a["sin"].t().contiguous().t()),
                    "fp32 contiguous tables"),
    "short_tables": (lambda a: a.update(cos=a["cos"][:8].contiguous(),
                                        sin=a["sin"][:8].contiguous()), "at least S rows"),
    "sin_other_shape": (lambda a: a.update(sin=a["sin"][:18].contiguous()), "one shape"),
    "wq_fp32": (lambda a: a.update(wq=a["wq"].float()), "norm weights"),
    "wk_length": (lambda a: a.update(wk=a["wk"][:32].contiguous()), "norm weights"),
    "wk_strided": (lambda a: a.update(wk=a["wk"].repeat(2)[::2]), "norm weights"),
    "q_unaligned": (lambda a: a.update(q=_unaligned(a["q"])), "16-byte aligned"),
    "k_unaligned": (lambda a: a.update(k=_unaligned(a["k"].contiguous())), "16-byte aligned"),
    "eps_negative": (lambda a: a.update(eps=-1e-6), "eps must be >= 0"),
}


@pytest.mark.parametrize("case", sorted(FWD_REJECTS))
def test_forward_rejects(case):
    a = _good()
    change, msg = FWD_REJECTS[case]
    change(a)
    with pytest.raises(RuntimeError, match=msg):
        hip.ext().qk_norm_rope_fwd(a["q"], a["k"], a["wq"], a["wk"], a["cos"], a["sin"],
                                   a["eps"])


BWD_REJECTS = {
    "invrms_fp64": (lambda b: b.update(iq=b["iq"].double()), "invrms"),
    "invrms_shape": (lambda b: b.update(ik=b["ik"].transpose(1, 2).contiguous()), "invrms"),
    "invrms_strided": (lambda b: b.update(iq=b["iq"].transpose(1, 2).contiguous()
                                          .transpose(1, 2)), "invrms"),
    "dqo_other_layout": (lambda b: b.update(dqo=b["dqo"].contiguous()), "layout of q"),
    "dko_fp32": (lambda b: b.update(dko=b["dko"].float()), "layout of q"),
    "q_fp32": (lambda b: b.update(q=b["q"].float()), "bf16"),
    "partial_rotary": (lambda b: b.update(cos=b["cos"][:, :32].contiguous(),
                                          sin=b["sin"][:, :32].contiguous()), "full rotary"),
}


@pytest.mark.parametrize("case", sorted(BWD_REJECTS))
def test_backward_rejects(case):
    a = _good()
    qo, ko, iq, ik = hip.ext().qk_norm_rope_fwd(a["q"], a["k"], a["wq"], a["wk"], a["cos"],
                                                a["sin"], a["eps"])
    b = dict(a, dqo=torch.ones_like(qo), dko=torch.ones_like(ko), iq=iq, ik=ik)
    assert b["dqo"].stride() == a["q"].stride()
    change, msg = BWD_REJECTS[case]
    change(b)
    with pytest.raises(RuntimeError, match=msg):
        hip.ext().qk_norm_rope_bwd(b["dqo"], b["dko"], b["q"], b["k"], b["wq"], b["wk"],
                                   b["iq"], b["ik"], b["cos"], b["sin"])


# -- 7. dispatch ----------------------------------------------------------------------------

@pytest.fixture
def spy(monkeypatch):
    calls = {"fwd": 0, "bwd": 0, "torch": 0}
    ext = hip.ext()
    real_fwd, real_bwd, real_torch = ext.qk_norm_rope_fwd, ext.qk_norm_rope_bwd, \
        Fn.qk_norm_rope_torch

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(ext, "qk_norm_rope_fwd", count("fwd", real_fwd))
    monkeypatch.setattr(ext, "qk_norm_rope_bwd", count("bwd", real_bwd))
    monkeypatch.setattr(Fn, "qk_norm_rope_torch", count("torch", real_torch))
    return calls


def _op_args(hd, dtype=torch.bfloat16, S=16):
    q = torch.randn(2, S, 4, hd, device="cuda").to(dtype).transpose(1, 2).requires_grad_()
    k = torch.randn(2, S, 2, hd, device="cuda").to(dtype).transpose(1, 2).requires_grad_()
    wq = torch.ones(hd, dtype=dtype, device="cuda", requires_grad=True)
    wk = torch.ones(hd, dtype=dtype, device="cuda", requires_grad=True)
    cos, sin = _tables(hd, S + 4)
    return q, k, wq, wk, cos, sin


@pytest.mark.parametrize("hd", [64, 128])
def test_dispatch_reaches_the_extension(hd, spy):
    q, k, wq, wk, cos, sin = _op_args(hd)
    qo, ko = ops.qk_norm_rope(q, k, wq, wk, cos, sin, 1e-6)
    (qo.float().sum() + ko.float().sum()).backward()
    assert spy == {"fwd": 1, "bwd": 1, "torch": 0}
    assert q.grad.shape == q.shape and wq.grad.dtype == torch.bfloat16
    want = ops.qk_norm_rope_torch(q.detach(), k.detach(), wq.detach(), wk.detach(), cos, sin,
                                  1e-6)
    # the torch composition rounds the tables to bf16: close, not equal
    assert (qo.float() - want[0].float()).abs().max() <= 0.05 * want[0].float().abs().max()


@pytest.mark.parametrize("case", ["hd52", "fp32", "position_ids", "partial_rotary"])
def test_dispatch_takes_the_torch_path(case, spy):
    hd = 52 if case == "hd52" else 64
    q, k, wq, wk, cos, sin = _op_args(hd, torch.float32 if case == "fp32" else torch.bfloat16)
    kw = {}
    if case == "position_ids":
        kw["position_ids"] = torch.arange(16, device="cuda").unsqueeze(0)
    if case == "partial_rotary":
        cos, sin = _tables(32, 20)
    qo, ko = ops.qk_norm_rope(q, k, wq, wk, cos, sin, 1e-6, **kw)
    (qo.float().sum() + ko.float().sum()).backward()
    assert spy == {"fwd": 0, "bwd": 0, "torch": 1}
    assert torch.isfinite(q.grad.float()).all() and wq.grad is not None


def test_disable_switch_in_child_process():
    """RELORA_AMD_DISABLE_OPS is read once per process"""
    for disabled, want in (("qk_norm", "fwd=0 torch=1"), ("", "fwd=1 torch=0")):
        env = dict(os.environ, RELORA_AMD_DISABLE_OPS=disabled)
        res = subprocess.run([sys.executable, os.path.join(HERE, "qk_norm_dispatch_worker.py")],
                             env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        assert want in res.stdout, (disabled, res.stdout)
