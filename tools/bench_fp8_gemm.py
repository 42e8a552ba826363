"""Per-launch A/B of the fp8 and MXFP4 frozen-W forwards against the bf16,
int8 and NF4 paths.

For each (M, N, K), r = 128, bias off: `quantize_rows_fp8` alone,
`fused_fp8_gemm` and `fused_mxfp4_gemm` alone, their sums with the quantiser,
against `F.linear` + `lora_add_nt_` (the composed bf16 path), `fused_lora_gemm`,
`fused_int8_gemm`, `fused_nf4_gemm` and the MXFP4 materialize arm
(`dequantize_rows_mxfp4` + `F.linear` + `lora_add_nt_`); the MXFP4 weight
quantiser and dequantiser on W [N, K] as well.  Each variant
is warmed up, then timed with device events in rounds that alternate the
variants; the figure is the median over rounds of the per-launch time.
The fp8 and MXFP4 results are checked against float64 on a 256-row slice first.
`--mem` adds the peak-HBM A/B of a training step (tools/bench_quant_mem.py).

  python tools/bench_fp8_gemm.py [--rounds 15] [--iters 20] [--mem]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch
import torch.nn.functional as F

from relora_amd.ops import hip

SHAPES = [(16384, 2048, 2048), (16384, 4096, 4096), (16384, 11008, 4096),
          (16384, 4096, 11008), (16384, 1024, 1024)]
BF = torch.bfloat16


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # us per launch


def bench_shape(M, N, K, r, rounds, iters):
    ext = hip.ext_or_raise()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    t = torch.randn(M, r, device="cuda", generator=g).to(BF)
    bw = (torch.randn(N, r, device="cuda", generator=g) * 0.1).to(BF)
    empty = x.new_empty(0)
    wq, ws = ext.quantize_rows_fp8(w)
    xq, xs = ext.quantize_rows_fp8(x)
    w8, a8 = ext.quantize_int8(w.view(-1))
    w4, a4 = ext.quantize_nf4(w.view(-1))
    wm, sm = ext.quantize_rows_mxfp4(w)

    # correctness at the timed size: first 256 rows against float64
    xd = ext.dequantize_rows_fp8(xq[:256].contiguous(), xs[:256].contiguous(), 256, K,
                                 torch.float32).double()
    lora = t[:256].double() @ bw.double().t()
    lora_abs = t[:256].double().abs() @ bw.double().abs().t()
    for name, y, wd in (
            ("fused_fp8_gemm", ext.fused_fp8_gemm(xq, xs, wq, ws, N, t, bw, empty, 1.0),
             ext.dequantize_rows_fp8(wq, ws, N, K, torch.float32)),
            ("fused_mxfp4_gemm", ext.fused_mxfp4_gemm(xq, xs, wm, sm, N, t, bw, empty, 1.0),
             ext.dequantize_rows_mxfp4(wm, sm, N, K, torch.float32))):
        wd = wd.double()
        ref = xd @ wd.t() + lora
        bound = 2.0 ** -8 * ref.abs() + (K + r) * 2.0 ** -23 * (xd.abs() @ wd.abs().t() + lora_abs)
        assert bool(((y[:256].double() - ref).abs() <= bound).all()), f"{name} is off at this shape"
    del xd, wd, ref, bound, y, lora, lora_abs

    def composed():
        out = F.linear(x, w)
        ext.lora_add_nt_(out, t, bw)

    def materialize_arm():
        out = F.linear(x, ext.dequantize_rows_mxfp4(wm, sm, N, K, BF))
        ext.lora_add_nt_(out, t, bw)

    variants = {
        "quantize_rows_fp8": lambda: ext.quantize_rows_fp8(x),
        "fused_fp8_gemm": lambda: ext.fused_fp8_gemm(xq, xs, wq, ws, N, t, bw, empty, 1.0),
        "linear+lora_add_nt": composed,
        "fused_lora_gemm": lambda: ext.fused_lora_gemm(x, w, t, bw, empty, 1.0),
        "fused_mxfp4_gemm": lambda: ext.fused_mxfp4_gemm(xq, xs, wm, sm, N, t, bw, empty, 1.0),
        "mxfp4_materialize_arm": materialize_arm,
        "fused_nf4_gemm": lambda: ext.fused_nf4_gemm(x, w4, a4, N, t, bw, empty, 1.0),
        "quantize_rows_mxfp4": lambda: ext.quantize_rows_mxfp4(w),
        "dequantize_rows_mxfp4": lambda: ext.dequantize_rows_mxfp4(wm, sm, N, K, BF),
    }
    if K % 256 == 0:
        variants["fused_int8_gemm"] = lambda: ext.fused_int8_gemm(x, w8, a8, N, t, bw, empty, 1.0)
    for fn in variants.values():
        timed(fn, 5)
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(timed(fn, iters))
    row = {"M": M, "N": N, "K": K, "r": r}
    for k, v in samples.items():
        row[k + "_us"] = round(statistics.median(v), 1)
        row[k + "_spread_us"] = [round(min(v), 1), round(max(v), 1)]
    row["fp8_sum_us"] = round(row["quantize_rows_fp8_us"] + row["fused_fp8_gemm_us"], 1)
    row["mxfp4_sum_us"] = round(row["quantize_rows_fp8_us"] + row["fused_mxfp4_gemm_us"], 1)
    row["fused_mxfp4_gemm_tflops"] = round(2.0 * M * N * (K + r) / row["fused_mxfp4_gemm_us"] / 1e6, 1)
    row["fused_fp8_gemm_tflops"] = round(2.0 * M * N * (K + r) / row["fused_fp8_gemm_us"] / 1e6, 1)
    row["quantize_rows_fp8_gbs"] = round(3.0 * M * K / row["quantize_rows_fp8_us"] / 1e3, 1)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--r", type=int, default=128)
    p.add_argument("--mem", action="store_true")
    p.add_argument("--model", default="configs/llama_1b.json")
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for M, N, K in SHAPES:
        print(json.dumps(bench_shape(M, N, K, args.r, args.rounds, args.iters)), flush=True)
    if args.mem:
        from bench_quant_mem import run
        for q in (None, "8bit", "fp8", "4bit", "mxfp4"):
            peak, dt, loss = run(args.model, 4, 2048, q)
            print(json.dumps({"model": args.model, "quantize": q, "peak_hbm_gib": round(peak, 2),
                              "ms_per_step": round(dt * 1e3), "loss": round(loss, 3)}), flush=True)


if __name__ == "__main__":
    main()
