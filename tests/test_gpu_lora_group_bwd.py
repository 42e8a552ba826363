"""Group LoRA backward kernels: lora_add_nn_group_ (one dx pass for all
siblings), skinny_grad_group (every dA from one read of x) and the
RELORA_AMD_LORA_GROUP_BWD switch of lora_group_bwd.  float64 CPU references,
masks from dropout_mask_fwd with the same seeds.  All @gpu.

Tolerances: those of tests/test_gpu_lora_group.py against float64
(0.05 * max(1, |ref|max) for dx, 0.03 * |ref|max + 0.05 for dA), and the group
kernel's max error is at most the sequential calls' max error on the same
inputs plus one bf16 ulp of |ref|max (2^-8 * |ref|max).
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from relora_amd.ops import hip
from relora_amd.ops.functional import _next_dropout_seed, set_dropout_rng_state

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lora_group_bwd_worker as worker  # noqa: E402

SEED_MASK = 0x7FFFFFFFFFFFFFFF
ULP = 2.0 ** -8


def ext():
    return hip.ext()


def unpack_mask(mask, M, K):
    mb = mask.view(M, K // 8)
    bits = torch.zeros(M, K, device=mask.device, dtype=torch.bool)
    for j in range(8):
        bits[:, j::8] = ((mb >> j) & 1).bool()
    return bits


def max_err(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item()


def make_inputs(M, K, r, G, p, seed, zero_out=False):
    """base[M,K] (the old dx, or x), Ps[g][M,r], Qs[g][r,K], masks (empty at
    p == 0) and their unpacked keep bits on the CPU."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    Ps = [(torch.randn(M, r, generator=g) * 0.1).to(torch.bfloat16).cuda() for _ in range(G)]
    Qs = [(torch.randn(r, K, generator=g) * 0.1).to(torch.bfloat16).cuda() for _ in range(G)]
    masks, keeps = [], []
    for i in range(G):
        if p > 0:
            _, mask = ext().dropout_mask_fwd(base, p, (0x1234567 * (i + 1) + seed) & SEED_MASK)
            masks.append(mask)
            keeps.append(unpack_mask(mask, M, K).cpu())
        else:
            keeps.append(torch.ones(M, K, dtype=torch.bool))
    if zero_out:
        base = torch.zeros_like(base)
    return base, Ps, Qs, masks, keeps


GRID = [(M, K, r, G) for M in (130, 192) for K in (256, 264)
        for r in (32, 64, 96, 128) for G in (1, 2, 3)]
EMPTY = dict(device="cuda", dtype=torch.uint8)


# -- 1. lora_add_nn_group_ -----------------------------------------------------

@pytest.mark.parametrize("M,K,r,G", GRID)
def test_add_nn_group(M, K, r, G):
    for p in (0.0, 0.5):
        out0, Ps, Qs, masks, keeps = make_inputs(M, K, r, G, p, seed=M + K + r + G)
        inv_keep = 1.0 / (1.0 - p)
        ref = out0.cpu().double()
        for g in range(G):
            lora = (Ps[g].cpu().double() @ Qs[g].cpu().double()) * inv_keep
            ref = ref + torch.where(keeps[g], lora, torch.zeros_like(lora))
        seq = out0.clone()
        for g in range(G):
            ext().lora_add_nn_(seq, Ps[g], Qs[g], masks[g] if p > 0 else torch.empty(0, **EMPTY),
                               inv_keep)
        got = out0.clone()
        ext().lora_add_nn_group_(got, Ps, Qs, masks, inv_keep)
        refmax = ref.abs().max().item()
        e_seq, e_got = max_err(seq, ref), max_err(got, ref)
        print(f"{(M, K, r, G)} p {p}: sequential err {e_seq:.3e} group err {e_got:.3e} "
              f"|ref|max {refmax:.3e}")
        assert e_got <= 0.05 * max(1.0, refmax), (p, e_got)
        assert e_got <= e_seq + ULP * refmax, (p, e_got, e_seq, refmax)


@pytest.mark.parametrize("M,K,r,G", [(130, 264, 96, 3), (192, 256, 128, 2)])
def test_add_nn_group_respects_every_mask(M, K, r, G):
    out, Ps, Qs, masks, keeps = make_inputs(M, K, r, G, 0.5, seed=77, zero_out=True)
    ext().lora_add_nn_group_(out, Ps, Qs, masks, 2.0)
    any_kept = keeps[0].clone()
    for k in keeps[1:]:
        any_kept |= k
    outc = out.cpu()
    assert abs((~any_kept).float().mean().item() - 0.5 ** G) < 0.02
    assert (outc[~any_kept] == 0).all()
    assert (outc[any_kept] != 0).float().mean() > 0.99


def test_add_nn_group_rejects_unsupported():
    out, Ps, Qs, masks, _ = make_inputs(130, 256, 64, 2, 0.5, seed=5)
    with pytest.raises(RuntimeError):   # non-contiguous out
        wide = torch.zeros(130, 512, device="cuda", dtype=torch.bfloat16)
        ext().lora_add_nn_group_(wide[:, :256], Ps, Qs, masks, 2.0)
    with pytest.raises(RuntimeError):   # unequal r
        ext().lora_add_nn_group_(out, [Ps[0], Ps[1][:, :32].contiguous()],
                                 [Qs[0], Qs[1][:32].contiguous()], masks, 2.0)


# -- 2. skinny_grad_group ------------------------------------------------------

def chunk_rows(M, C):
    """rows per M-chunk under the chunk rule of skinny_grad"""
    chunks, ctiles = 1, (C + 127) // 128
    while chunks < 32 and ctiles * chunks < 512 and (M + chunks - 1) // chunks > 256:
        chunks <<= 1
    rows = (M + chunks - 1) // chunks
    return (rows + 63) // 64 * 64


def grad_reference(Ps, x, keeps, inv_keep):
    xd = x.cpu().double()
    return [P.cpu().double().t() @ (xd * k.double() * inv_keep) for P, k in zip(Ps, keeps)]


def check_grad_group(Ps, x, masks, keeps, p, dtype):
    inv_keep = 1.0 / (1.0 - p)
    refs = grad_reference(Ps, x, keeps, inv_keep)
    got = ext().skinny_grad_group(Ps, x, masks, inv_keep, dtype)
    assert len(got) == len(Ps)
    for g, ref in enumerate(refs):
        seq = ext().skinny_grad(Ps[g], x, masks[g] if p > 0 else torch.empty(0, **EMPTY),
                                inv_keep, 1.0, False, dtype)
        assert got[g].dtype == dtype and got[g].shape == seq.shape
        refmax = ref.abs().max().item()
        e_seq, e_got = max_err(seq, ref), max_err(got[g], ref)
        print(f"sibling {g} p {p} {dtype}: sequential err {e_seq:.3e} group err {e_got:.3e} "
              f"|ref|max {refmax:.3e}")
        assert e_got <= 0.03 * refmax + 0.05, (g, e_got)
        assert e_got <= e_seq + ULP * refmax, (g, e_got, e_seq, refmax)
        # same chunks, m-tiles and MFMA order per sibling: the same bits
        assert torch.equal(got[g], seq), g


@pytest.mark.parametrize("M,K,r,G", GRID + [(1100, K, r, G) for K in (256, 264)
                                             for r in (32, 64, 96, 128) for G in (1, 2, 3)])
def test_skinny_grad_group(M, K, r, G):
    if M == 1100:  # several chunks, the last one short
        rows = chunk_rows(M, K)
        assert M > 2 * rows and M % rows not in (0, rows)
    for p in (0.0, 0.5):
        x, Ps, _, masks, keeps = make_inputs(M, K, r, G, p, seed=M + K + r + G + 1)
        for dtype in (torch.bfloat16, torch.float32):
            check_grad_group(Ps, x, masks, keeps, p, dtype)


@pytest.mark.parametrize("which", ["second", "last"])
@pytest.mark.parametrize("K,r,G", [(264, 96, 3), (256, 128, 2)])
def test_skinny_grad_group_chunk_isolation(K, r, G, which):
    """P is zero outside one chunk: only that chunk's rows of x contribute,
    also where the chunk ends inside an m-tile (the short last chunk)."""
    M, p = 1100, 0.5
    rows = chunk_rows(M, K)
    lo = rows if which == "second" else (M - 1) // rows * rows
    hi = min(M, lo + rows)
    x, Ps, _, masks, keeps = make_inputs(M, K, r, G, p, seed=K + r + G)
    for P in Ps:
        P[:lo] = 0
        P[hi:] = 0
    refs = [P[lo:hi].cpu().double().t() @ (x[lo:hi].cpu().double() * k[lo:hi].double() * 2.0)
            for P, k in zip(Ps, keeps)]
    got = ext().skinny_grad_group(Ps, x, masks, 2.0, torch.float32)
    for g, ref in enumerate(refs):
        refmax = ref.abs().max().item()
        assert refmax > 0
        assert max_err(got[g], ref) <= 0.03 * refmax + 0.05
        assert max_err(got[g], ref) <= 1e-3 * refmax   # fp32 output of bf16 products


# -- 3. op level: the switch on and off, one child process each ------------------

def run_worker(tmp_path, switch):
    out = tmp_path / f"bwd{switch}.pt"
    env = dict(os.environ, RELORA_AMD_LORA_GROUP_BWD=switch)
    res = subprocess.run([sys.executable, os.path.join(HERE, "lora_group_bwd_worker.py"),
                          str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def worker_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora_group_bwd")
    return run_worker(d, "1"), run_worker(d, "0")


def op_reference(case):
    """float64 dx and dA on the CPU, with the masks the philox stream yields."""
    c = worker.CASES[case]
    x, specs, dys = worker.make_group(c["M"], c["K"], c["Ns"], c["r"], worker.SEED)
    torch.manual_seed(worker.TORCH_SEED)
    set_dropout_rng_state(worker.C0)
    seeds = [_next_dropout_seed() & SEED_MASK for _ in specs]
    x64 = x.cpu().double().requires_grad_(True)
    ys, As = [], []
    for (W, A, B), seed in zip(specs, seeds):
        _, mask = ext().dropout_mask_fwd(x, worker.P, seed)
        keep = unpack_mask(mask, c["M"], c["K"]).cpu()
        A64 = A.cpu().double().requires_grad_(True)
        xd = x64 * keep.double() / (1.0 - worker.P)
        ys.append(x64 @ W.cpu().double().t()
                  + worker.SCALE * (xd @ A64.t()) @ B.cpu().double().t())
        As.append(A64)
    torch.autograd.backward(ys, [d.cpu().double() for d in dys])
    return x64.grad, [a.grad for a in As]


@pytest.mark.parametrize("case", sorted(worker.CASES))
def test_switch_on_matches_off(worker_results, case):
    on, off = worker_results
    assert on["switch"] is True and off["switch"] is False
    a, b = on["cases"][case], off["cases"][case]
    for ya, yb in zip(a["ys"], b["ys"]):
        assert torch.equal(ya, yb)
    for da, db in zip(a["dBs"], b["dBs"]):
        assert torch.equal(da, db)
    rdx, rdAs = op_reference(case)
    refmax = rdx.abs().max().item()
    e_on, e_off = max_err(a["dx"], rdx), max_err(b["dx"], rdx)
    print(f"{case} dx: off err {e_off:.3e} on err {e_on:.3e} |ref|max {refmax:.3e}")
    assert e_on <= 0.05 * max(1.0, refmax)
    assert e_on <= e_off + ULP * refmax
    for g, ref in enumerate(rdAs):
        refmax = ref.abs().max().item()
        e_on, e_off = max_err(a["dAs"][g], ref), max_err(b["dAs"][g], ref)
        print(f"{case} dA[{g}]: off err {e_off:.3e} on err {e_on:.3e} |ref|max {refmax:.3e}")
        assert e_on <= 0.03 * refmax + 0.05
        assert e_on <= e_off + ULP * refmax
