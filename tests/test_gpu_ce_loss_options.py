"""GPU tests of the z-loss / label-smoothing variants of the fused
cross-entropy: the two HIP kernels, the op end to end, and the model.

Per valid row (logits x, p = softmax(x), target t, lse = log sum exp x):
    loss_row      = lse - (1-eps)*x_t - (eps/V)*sum_j x_j + z*lse^2
    dloss_row/dx_j = (1 + 2*z*lse)*p_j - (1-eps)*[j == t] - eps/V

Kernel references are float64 from the same already-rounded inputs.
Tolerances for kernel outputs, |got - ref| <= atol + rtol*|ref| elementwise:
  fp32 outputs  rtol 1e-4,  atol 1e-6
  bf16 outputs  rtol 2^-7,  atol 1e-6*gscale   (round-to-nearest is 2^-9; the
                rest covers __expf and the fp32 reductions)
The row sum is compared relative to the sum itself, so the kernel-grid rows
have a non-zero mean (1.5): a zero-mean row's sum is a cancellation whose
fp32 error is relative to sum|x|, not to |sum x|.

End-to-end tolerances are the ones of test_fused_ce_end_to_end_gpu (bf16
GEMMs): loss atol 3e-2, gradients atol 1e-3 / rtol 5e-2."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

M_ROWS = 16
IGNORED = (2, 9)
OPTIONS = [(1e-2, 0.0), (0.0, 0.25), (1e-2, 0.25)]


def ext():
    from relora_amd.ops import hip

    e = hip.ext()
    assert e is not None, "HIP extension not built"
    return e


def assert_close(got, ref64, out_dtype, gscale=1.0, what=""):
    if out_dtype == torch.bfloat16:
        rtol, atol = 2.0 ** -7, 1e-6 * gscale
    else:
        rtol, atol = 1e-4, 1e-6
    got = got.double()
    err = (got - ref64).abs()
    bad = err > atol + rtol * ref64.abs()
    i = err.argmax().item()
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs err {err.max().item():.3e} "
        f"at {i} (got {got.flatten()[i].item():.6e}, ref {ref64.flatten()[i].item():.6e})")


@functools.lru_cache(maxsize=None)
def _case(V, dtype, shift):
    """Rounded logits, labels and the float64 row statistics, computed once
    per (V, dtype, shift) and shared by every test; never modified."""
    g = torch.Generator(device="cpu").manual_seed(1000 + V)
    logits = (torch.randn(M_ROWS, V, generator=g) * 2 + 1.5 + shift).to(dtype).cuda()
    labels = torch.randint(0, V, (M_ROWS,), generator=g)
    labels[0] = 0          # first column of the vector body
    labels[1] = V - 1      # inside the scalar tail
    for r in IGNORED:
        labels[r] = -100
    labels = labels.cuda()
    x = logits.double()
    lse = torch.logsumexp(x, -1)
    valid = labels != -100
    tgt = x.gather(1, labels.clamp_min(0).unsqueeze(1)).squeeze(1)
    tgt = torch.where(valid, tgt, torch.zeros_like(tgt))
    return logits, labels, lse, tgt, x.sum(-1)


def _ref_grad(logits, labels, lse, z, eps, gscale):
    x = logits.double()
    V = x.shape[1]
    valid = labels != -100
    g = (1 + 2 * z * lse).unsqueeze(1) * torch.exp(x - lse.unsqueeze(1)) - eps / V
    g[valid, labels[valid]] -= 1 - eps
    g[~valid] = 0
    return g * gscale


def _check_kernels(V, dtype, z, eps, shift, gscale=1.0):
    logits, labels, ref_lse, ref_tgt, ref_sum = _case(V, dtype, shift)
    lse, tgt, rsum = ext().ce_row_stats_ex(logits, labels, -100)
    assert lse.dtype == tgt.dtype == rsum.dtype == torch.float32
    assert_close(lse, ref_lse, torch.float32, what="lse")
    assert_close(tgt, ref_tgt, torch.float32, what="tgt")
    assert_close(rsum, ref_sum, torch.float32, what="row sum")
    for r in IGNORED:
        assert tgt[r].item() == 0.0

    buf = logits.clone()
    ext().ce_grad_ex_(buf, labels, lse, gscale, z, eps, -100)
    ref = _ref_grad(logits, labels, ref_lse, z, eps, gscale)
    assert_close(buf, ref, dtype, gscale=gscale, what="grad")
    for r in IGNORED:
        assert torch.equal(buf[r], torch.zeros_like(buf[r])), f"ignored row {r} not zero"
    # the cases bite: the plain gradient is not within tolerance of this one
    plain = _ref_grad(logits, labels, ref_lse, 0.0, 0.0, gscale)
    assert ((plain - ref).abs() > 4 * (1e-6 * gscale + 2.0 ** -7 * ref.abs())).any()


@pytest.mark.parametrize("z,eps", OPTIONS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [50, 101, 4104, 32100])
def test_kernels(V, dtype, z, eps):
    _check_kernels(V, dtype, z, eps, shift=0.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [101, 32100])
def test_kernels_shifted_rows(V, dtype):
    """+30 on every logit: lse is about 40, so (1 + 2*z*lse) is about 1.8,
    and the row sum is about 31.5*V."""
    _, _, ref_lse, _, _ = _case(V, dtype, 30.0)
    assert 35 < ref_lse.min().item() and ref_lse.max().item() < 50
    _check_kernels(V, dtype, 1e-2, 0.25, shift=30.0)


def test_kernel_gscale():
    """gscale multiplies every term, the uniform eps/V one included."""
    _check_kernels(4104, torch.bfloat16, 1e-2, 0.25, shift=0.0, gscale=0.125)
    _check_kernels(4104, torch.float32, 1e-2, 0.25, shift=0.0, gscale=0.125)


def test_host_checks():
    logits, labels, lse, _, _ = _case(101, torch.float32, 0.0)
    lse = lse.float()
    buf = logits.clone()
    with pytest.raises(RuntimeError):
        ext().ce_grad_ex_(buf, labels, lse, 1.0, -1e-3, 0.0, -100)
    with pytest.raises(RuntimeError):
        ext().ce_grad_ex_(buf, labels, lse, 1.0, 0.0, 1.0, -100)
    with pytest.raises(RuntimeError):
        ext().ce_grad_ex_(buf, labels, lse, 1.0, 0.0, -0.1, -100)
    with pytest.raises(RuntimeError):
        ext().ce_grad_ex_(buf, labels[:-1].contiguous(), lse, 1.0, 1e-2, 0.0, -100)
    with pytest.raises(RuntimeError):
        ext().ce_row_stats_ex(buf, labels.int(), -100)
    assert torch.equal(buf, logits)  # nothing was launched


# ---------------------------------------------------------------------------
# op, end to end
# ---------------------------------------------------------------------------

E2E_M, E2E_H, E2E_V = 512, 256, 32100
E2E_OPTIONS = [(1e-2, 0.0), (0.0, 0.1), (1e-2, 0.1)]
# backward of loss * GRAD_SCALE.  The gradient atol is absolute, and at scale 1
# every dw element off the target rows (~3e-5 * sqrt(M) / M) sits far below it.
# At 16 * M those elements are ~0.015, where z's 20% change of the softmax part
# is outside the tolerance (test_e2e_inputs_are_conditioned checks that).
GRAD_SCALE = 16.0 * E2E_M


def _ref_objective(h, w, labels, z, eps):
    logits = h @ w.t()
    lse = torch.logsumexp(logits, -1)
    valid = labels != -100
    zl = z * (lse[valid] ** 2).mean()
    loss = F.cross_entropy(logits, labels, label_smoothing=eps, ignore_index=-100) + zl
    return loss, F.cross_entropy(logits, labels, ignore_index=-100).detach(), zl.detach()


@functools.lru_cache(maxsize=None)
def _e2e_inputs():
    """bf16 hidden/weight whose target logit sits 4 above a zero-mean row, so
    smoothing moves the loss by eps*(x_t - mean x) ~ 0.4 (with random labels
    that shift averages to ~0); lse ~ ln V ~ 10.4, so z = 1e-2 moves it by ~1."""
    g = torch.Generator(device="cpu").manual_seed(7)
    weight = torch.randn(E2E_V, E2E_H, generator=g) * 0.02
    # distinct targets: two rows sharing one would cancel in its dw row, and the
    # bf16 rounding of the two ~-GRAD_SCALE/M dlogits would not
    labels = torch.randperm(E2E_V, generator=g)[:E2E_M]
    labels[3] = -100
    labels[200] = -100
    wt = weight[labels.clamp_min(0)]
    hidden = torch.randn(E2E_M, E2E_H, generator=g) + 4.0 * wt / (wt * wt).sum(-1, keepdim=True)
    return hidden.bfloat16().cuda(), weight.bfloat16().cuda(), labels.cuda()


@functools.lru_cache(maxsize=None)
def _e2e_reference(z, eps):
    """fp32 torch reference: (loss, ce, zl, dh, dw) for loss * GRAD_SCALE."""
    hidden, weight, labels = _e2e_inputs()
    h = hidden.float().requires_grad_(True)
    w = weight.float().requires_grad_(True)
    loss, ce, zl = _ref_objective(h, w, labels, z, eps)
    (loss * GRAD_SCALE).backward()
    return loss.detach(), ce, zl, h.grad, w.grad


def _grads_close(got, ref):
    return (got.float() - ref).abs() <= 1e-3 + 5e-2 * ref.abs()


def test_e2e_inputs_are_conditioned():
    """Each option moves the reference loss by >= 10x the loss tolerance, and
    the plain gradients are outside the gradient tolerance of each option's.
    (z-loss alone cannot show in dh here: it scales the softmax part, whose
    image under W is E_p[w] ~ 1e-4 next to the target's w_t ~ 2e-2.  It shows
    in dw; smoothing shows in both.)"""
    plain = _e2e_reference(0.0, 0.0)
    for z, eps in E2E_OPTIONS:
        ref = _e2e_reference(z, eps)
        assert (ref[0] - plain[0]).item() >= 10 * 3e-2, (z, eps, ref[0], plain[0])
        assert not _grads_close(plain[4], ref[4]).all(), (z, eps)
        if eps:
            assert not _grads_close(plain[3], ref[3]).all(), (z, eps)


def _run_e2e(z, eps):
    from relora_amd import ops as fops

    hidden, weight, labels = _e2e_inputs()
    h = hidden.clone().requires_grad_(True)
    w = weight.clone().requires_grad_(True)
    loss, ce, zl = fops.fused_cross_entropy(h, w, labels, z_loss=z, label_smoothing=eps,
                                            return_parts=True)
    assert not ce.requires_grad and not zl.requires_grad
    (loss * GRAD_SCALE).backward()
    ref_loss, ref_ce, ref_zl, ref_dh, ref_dw = _e2e_reference(z, eps)
    print(f"z={z} eps={eps}: loss {loss.item():.5f} ref {ref_loss.item():.5f}  "
          f"ce {ce.item():.5f} ref {ref_ce.item():.5f}  zl {zl.item():.5f} ref {ref_zl.item():.5f}  "
          f"dh err {(h.grad.float() - ref_dh).abs().max().item():.3e}  "
          f"dw err {(w.grad.float() - ref_dw).abs().max().item():.3e}")
    assert torch.allclose(loss.float(), ref_loss, atol=3e-2), (loss, ref_loss)
    assert torch.allclose(ce.float(), ref_ce, atol=3e-2), (ce, ref_ce)
    assert torch.allclose(zl.float(), ref_zl, atol=3e-2), (zl, ref_zl)
    assert _grads_close(h.grad, ref_dh).all(), "dh"
    assert _grads_close(w.grad, ref_dw).all(), "dw"
    for r in (3, 200):
        assert torch.equal(h.grad[r], torch.zeros_like(h.grad[r]))


@pytest.mark.parametrize("z,eps", E2E_OPTIONS)
def test_fused_ce_options_end_to_end(z, eps):
    _run_e2e(z, eps)


def test_fused_ce_options_multi_chunk(monkeypatch):
    import relora_amd.ops.functional as fn

    monkeypatch.setattr(fn, "_CE_CHUNK", 128)  # 4 chunks, fp32 dw_acc
    _run_e2e(1e-2, 0.1)


def test_fused_ce_options_recompute_logits(monkeypatch):
    import relora_amd.ops.functional as fn

    monkeypatch.setattr(fn, "_CE_SAVE_LOGITS", False)
    _run_e2e(1e-2, 0.1)


def test_off_path_is_untouched():
    from relora_amd import ops as fops

    hidden, weight, labels = _e2e_inputs()
    res = []
    for kw in ({}, {"z_loss": 0.0, "label_smoothing": 0.0}):
        h = hidden.clone().requires_grad_(True)
        w = weight.clone().requires_grad_(True)
        loss = fops.fused_cross_entropy(h, w, labels, **kw)
        loss.backward()
        res.append((loss.detach(), h.grad, w.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------


def test_llama_loss_options_gpu():
    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=32100, hidden_size=128, intermediate_size=352,
                      num_hidden_layers=2, num_attention_heads=4,
                      max_position_embeddings=128, rms_norm_eps=1e-6)
    model = LlamaForCausalLM(cfg).to(device="cuda", dtype=torch.bfloat16)
    x = torch.randint(0, cfg.vocab_size, (2, 64), device="cuda")
    z, eps = 1e-2, 0.1

    model.eval()
    with torch.no_grad():
        plain_eval = model(input_ids=x, labels=x).loss
    model.set_loss_options(z_loss=z, label_smoothing=eps)
    with torch.no_grad():
        assert torch.equal(model(input_ids=x, labels=x).loss, plain_eval)

    model.train()
    fused = model(input_ids=x, labels=x)
    model.fused_ce = False
    unfused = model(input_ids=x, labels=x)
    assert torch.allclose(fused.loss.float(), unfused.loss.float(), atol=3e-2), \
        (fused.loss, unfused.loss)
    assert not fused.ce_loss.requires_grad and not fused.z_loss.requires_grad
    # z * lse^2 ~ 1e-2 * ln(V)^2 ~ 1: far above the tolerance
    assert fused.z_loss.item() > 0.5

    # loss = ce + eps * mean(x_t - mean_j x_j) + zl, smoothing term from the logits
    logits = unfused.logits[:, :-1].reshape(-1, cfg.vocab_size).detach().float()
    tgt = logits.gather(1, x[:, 1:].reshape(-1, 1)).squeeze(1)
    smooth = eps * (tgt - logits.mean(-1)).mean()
    total = fused.ce_loss.float() + smooth + fused.z_loss.float()
    assert torch.allclose(total, fused.loss.float(), atol=3e-2), (total, fused.loss)
    fused.loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
