"""The MXFP4 backward on the MI355X: the input-gradient arm `quantize_rows_fp8` +
stripe exponents + `fused_mxfp4_gemm_dx` against the arm it replaces,
`dequantize_rows_mxfp4` (the materialize of `--quantize mxfp4`) + `dy @ w`.

  python tools/bench_mxfp4_dx.py [--rounds 15] [--iters 20] [--shapes 0,1,2,3]
      per (M, N, K): each launch alone and the two arms, alternating, medians
      with min/max over the rounds; the materialize arm is timed twice a round,
      its second series over its first is the repeat spread of the ratio.  The
      arm is checked against float64 on a 256-row slice first.  The stripe
      exponents are recomputed in every call of the arm (the module caches them).
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

BF, E4 = torch.bfloat16, torch.float8_e4m3fn
# M = 16 sequences of 1024; (N, K) of llama_1b, llama_7b attention, 7b down, 7b gate/up
SHAPES = [(16384, 2048, 2048), (16384, 4096, 4096), (16384, 4096, 11008), (16384, 11008, 4096)]


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def bench_shape(M, N, K, rounds, iters):
    from relora_amd.ops import hip
    from relora_amd.ops.quant import transcode_mxfp4_e4m3_ref
    ext = hip.ext_or_raise()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    dy = torch.randn(M, N, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    wq, ws = ext.quantize_rows_mxfp4(w)
    emax = ws.amax(dim=0)
    gq, gs = ext.quantize_rows_fp8(dy)

    # float64 on a slice: the arm against its own operands, and against the bf16 arm
    dx = ext.fused_mxfp4_gemm_dx(gq, gs, wq, ws, emax, N, K)[:256].double()
    gd = gq[:256].view(E4).double() * (gs[:256].double() / 448)[:, None]
    b, e = (v.cuda() for v in transcode_mxfp4_e4m3_ref(wq.cpu(), ws.cpu(), K))
    assert torch.equal(e, emax)
    bd = b.view(E4).float().double() * torch.exp2(e.double() - 133).repeat_interleave(32)
    ref = gd @ bd
    assert bool(((dx - ref).abs() <= 2.0 ** -8 * ref.abs() + N * 2.0 ** -23 * (gd.abs() @ bd.abs())).all())
    full = dy[:256].double() @ ext.dequantize_rows_mxfp4(wq, ws, N, K, torch.float32).double()
    rel = float((dx - full).norm() / full.norm())
    del b, bd, ref, full

    def mxfp4_arm():
        a, s = ext.quantize_rows_fp8(dy)
        ext.fused_mxfp4_gemm_dx(a, s, wq, ws, ws.amax(dim=0), N, K)

    def materialize_arm():
        dy @ ext.dequantize_rows_mxfp4(wq, ws, N, K, BF)

    wd = ext.dequantize_rows_mxfp4(wq, ws, N, K, BF)
    variants = {
        "quantize_rows_fp8": lambda: ext.quantize_rows_fp8(dy),
        "stripe_emax": lambda: ws.amax(dim=0),
        "fused_mxfp4_gemm_dx": lambda: ext.fused_mxfp4_gemm_dx(gq, gs, wq, ws, emax, N, K),
        "dequantize_rows_mxfp4": lambda: ext.dequantize_rows_mxfp4(wq, ws, N, K, BF),
        "dy@w": lambda: dy @ wd,
        "materialize_arm": materialize_arm,
        "mxfp4_arm": mxfp4_arm,
        "materialize_arm_again": materialize_arm,
    }
    for fn in variants.values():
        timed(fn, 5)
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(timed(fn, iters))
    row = {"M": M, "N": N, "K": K, "rel_err_vs_bf16_arm": round(rel, 5)}
    for k, v in samples.items():
        row[k + "_us"] = round(statistics.median(v), 1)
        row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
    row["mxfp4_over_materialize"] = round(row["mxfp4_arm_us"] / row["materialize_arm_us"], 3)
    row["materialize_again_over_materialize"] = round(
        row["materialize_arm_again_us"] / row["materialize_arm_us"], 3)
    row["fused_mxfp4_gemm_dx_tflops"] = round(2.0 * M * N * K / row["fused_mxfp4_gemm_dx_us"] / 1e6, 1)
    row["dy@w_tflops"] = round(2.0 * M * N * K / row["dy@w_us"] / 1e6, 1)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--shapes", default="0,1,2,3", help="indices into SHAPES")
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for i in (int(s) for s in args.shapes.split(",")):
        print(json.dumps(bench_shape(*SHAPES[i], args.rounds, args.iters)), flush=True)


if __name__ == "__main__":
    main()
