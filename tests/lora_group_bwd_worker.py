"""Child-process worker for tests/test_gpu_lora_group_bwd.py.

RELORA_AMD_LORA_GROUP_BWD is read once at import, so the group backward
kernels on and off each need a fresh process.  `python
tests/lora_group_bwd_worker.py OUT.pt` runs lora_linear_group forward and
backward for every case of CASES under whatever environment it was started
with and saves {switch, cases: {name: {ys, dx, dAs, dBs}}} to OUT.pt.

The test module imports CASES, make_group and the run constants from here, so
both sides build the same inputs.
"""

import os
import sys

import torch

# the shapes of GROUP_CASES in tests/test_gpu_lora_group.py
CASES = {
    "aligned_g3": dict(M=192, K=256, Ns=(256, 256, 256), r=64),
    "odd_n_g2": dict(M=192, K=256, Ns=(333, 333), r=64),
    "aligned_g3_r32": dict(M=192, K=256, Ns=(256, 256, 256), r=32),
}
SCALE, P, C0, SEED = 0.5, 0.1, 1000, 21
TORCH_SEED = 11  # the dropout seeds mix in torch.initial_seed()


def make_group(M, K, Ns, r, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    specs = []
    for N in Ns:
        W = torch.randn(N, K, generator=g) * 0.05
        A = torch.randn(r, K, generator=g) * 0.05
        B = torch.randn(N, r, generator=g) * 0.05
        specs.append([t.to(torch.bfloat16).cuda() for t in (W, A, B)])
    dys = [torch.randn(M, N, generator=g).to(torch.bfloat16).cuda() for N in Ns]
    return x, specs, dys


def main(out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd.ops import functional as Fn
    from relora_amd.ops.functional import lora_linear_group, set_dropout_rng_state

    assert torch.cuda.is_available(), "lora group bwd worker needs a GPU"
    torch.manual_seed(TORCH_SEED)
    results = {}
    for name, c in CASES.items():
        x, specs, dys = make_group(c["M"], c["K"], c["Ns"], c["r"], SEED)
        x = x.requires_grad_(True)
        leaves = [[W, A.requires_grad_(True), B.requires_grad_(True)] for W, A, B in specs]
        set_dropout_rng_state(C0)
        ys = lora_linear_group(x, [(W, None, A, B, SCALE) for W, A, B in leaves],
                               dropout_p=P, training=True)
        torch.autograd.backward(ys, dys)
        results[name] = {
            "ys": [y.detach().cpu() for y in ys],
            "dx": x.grad.cpu(),
            "dAs": [l[1].grad.cpu() for l in leaves],
            "dBs": [l[2].grad.cpu() for l in leaves],
        }
    torch.cuda.synchronize()
    torch.save({"switch": Fn._LORA_GROUP_BWD, "cases": results}, out_path)
    print("LORA_GROUP_BWD_WORKER_DONE", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
