"""Norm kernels on the MI355X: stand-alone time per call of the extension
entries of norms.hip, against the one-read-one-write HBM time of the tensors
they must touch.

  python tools/bench_norms.py [--M 16384] [--H 768] [--dtype bf16]
                              [--ops layernorm_fwd,rmsnorm_fwd,...]
                              [--baseline-ext PATH/_relora_hip*.so]

With --baseline-ext a second build of the extension (the parent commit's, say)
is loaded next to the tree's own and the two alternate, --rounds times, on
the same tensors; the outputs of the two are compared first and the largest
difference is reported.  One JSON line.
"""

import argparse
import importlib.util
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

HBM_BYTES_PER_S = 8.0e12  # MI355X peak; the achievable streaming rate is lower
OPS = ("rmsnorm_fwd", "rmsnorm_bwd", "layernorm_fwd", "layernorm_bwd")
# [M, H] tensors read + written per call; the [H] and [M] vectors are noise
PASSES = {"rmsnorm_fwd": 2, "rmsnorm_bwd": 3, "layernorm_fwd": 2, "layernorm_bwd": 3}


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def _load(path):
    spec = importlib.util.spec_from_file_location("_relora_hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _calls(ext, a):
    y, ir = ext.rmsnorm_fwd(a["x"], a["w"], 1e-6)
    _, mean, invstd = ext.layernorm_fwd(a["x"], a["w"], a["b"], 1e-5)
    return {
        "rmsnorm_fwd": lambda: ext.rmsnorm_fwd(a["x"], a["w"], 1e-6),
        "rmsnorm_bwd": lambda: ext.rmsnorm_bwd(a["x"], a["w"], ir, a["dy"]),
        "layernorm_fwd": lambda: ext.layernorm_fwd(a["x"], a["w"], a["b"], 1e-5),
        "layernorm_bwd": lambda: ext.layernorm_bwd(a["x"], a["w"], mean, invstd, a["dy"]),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--M", type=int, default=16384)
    p.add_argument("--H", type=int, default=768)
    p.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("--ops", type=str, default=",".join(OPS))
    p.add_argument("--baseline-ext", type=str, default=None)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--rounds", type=int, default=7)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_norms.py measures on a GPU; none is available")
    from relora_amd.ops import hip

    names = [n for n in args.ops.split(",") if n]
    assert all(n in OPS for n in names), names
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    M, H = args.M, args.H
    a = {"x": torch.randn(M, H, device="cuda").to(dtype),
         "dy": torch.randn(M, H, device="cuda").to(dtype),
         "w": (1 + 0.1 * torch.randn(H, device="cuda")).to(dtype),
         "b": (0.1 * torch.randn(H, device="cuda")).to(dtype)}
    sides = {"tree": _calls(hip.ext(), a)}
    out = {"shape": [M, H], "dtype": args.dtype, "iters": args.iters, "rounds": args.rounds}
    if args.baseline_ext:
        sides["baseline"] = _calls(_load(args.baseline_ext), a)
        out["max_abs_diff"] = {
            n: max((u.float() - v.float()).abs().max().item()
                   for u, v in zip(sides["tree"][n](), sides["baseline"][n]()))
            for n in names}
    res = {(s, n): [] for s in sides for n in names}
    for _ in range(args.rounds):
        for n in names:
            for s in sides:
                res[(s, n)].append(_time(sides[s][n], args.iters, args.warmup))
    elem = a["x"].element_size()
    for n in names:
        out[n] = {"hbm_floor_us": round(PASSES[n] * M * H * elem / HBM_BYTES_PER_S * 1e6, 1)}
        for s in sides:
            v = sorted(res[(s, n)])
            out[n][s + "_us"] = {"min": round(v[0], 1), "median": round(v[len(v) // 2], 1),
                                 "max": round(v[-1], 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
