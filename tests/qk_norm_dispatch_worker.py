"""Child-process worker for tests/test_gpu_qk_norm_rope.py.

RELORA_AMD_DISABLE_OPS is parsed once per process, so the `qk_norm` switch
needs a fresh one.  Runs one ops.qk_norm_rope forward + backward at head_dim
64 under whatever environment it was started with and prints how often the
extension entry and the torch composition were entered."""

import os
import sys

import torch


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd import ops
    from relora_amd.ops import functional as Fn
    from relora_amd.ops import hip

    assert torch.cuda.is_available(), "qk_norm dispatch worker needs a GPU"
    calls = {"fwd": 0, "torch": 0}
    ext = hip.ext_or_raise()
    real_fwd, real_torch = ext.qk_norm_rope_fwd, Fn.qk_norm_rope_torch

    def fwd(*a, **kw):
        calls["fwd"] += 1
        return real_fwd(*a, **kw)

    def composed(*a, **kw):
        calls["torch"] += 1
        return real_torch(*a, **kw)

    ext.qk_norm_rope_fwd = fwd
    Fn.qk_norm_rope_torch = composed

    torch.manual_seed(0)
    hd, S = 64, 16
    q = torch.randn(2, S, 4, hd, device="cuda").bfloat16().transpose(1, 2).requires_grad_()
    k = torch.randn(2, S, 2, hd, device="cuda").bfloat16().transpose(1, 2).requires_grad_()
    wq = torch.ones(hd, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    wk = torch.ones(hd, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    cos, sin = (t.cuda() for t in ops.build_rope_cache(hd, S))
    qo, ko = ops.qk_norm_rope(q, k, wq, wk, cos, sin, 1e-6)
    (qo.float().sum() + ko.float().sum()).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(q.grad.float()).all() and torch.isfinite(wq.grad.float()).all()
    print(f"fwd={calls['fwd']} torch={calls['torch']}")


if __name__ == "__main__":
    main()
