"""The fp8 backward on the MI355X: the input-gradient pair
`quantize_rows_fp8_scaled` + `fused_fp8_gemm_dx` against the arm it replaces,
`dequantize_rows_fp8` (the materialize of `--quantize fp8`) + `dy @ w`.

  python tools/bench_fp8_dx.py kernel [--rounds 15] [--iters 20]
      per (M, N, K): each launch alone and the two arms, alternating, medians
      with min/max over the rounds; the GEMM alone in FLOP/s.  The pair is
      checked against float64 on a 256-row slice first.
  python tools/bench_fp8_dx.py model [--model configs/llama_250m.json] [--bs 8] [--steps 20]
      ReLoRA training steps with quantize="fp8", the switch off and on,
      alternating: tokens/s, peak memory and the loss after the same steps.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

BF = torch.bfloat16
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
    ext = hip.ext_or_raise()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    dy = torch.randn(M, N, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    wq, ws = ext.quantize_rows_fp8(w)
    gq, gs = ext.quantize_rows_fp8_scaled(dy, ws)

    # float64 on a slice: the pair against its own operands, and against the bf16 arm
    dx = ext.fused_fp8_gemm_dx(gq, gs, wq, K)[:256].double()
    gd = gq[:256].view(torch.float8_e4m3fn).double() * (gs[:256].double() / 448)[:, None]
    ref = gd @ wq.view(torch.float8_e4m3fn).double()
    assert bool(((dx - ref).abs() <= 2.0 ** -8 * ref.abs() + N * 2.0 ** -23
                 * (gd.abs() @ wq.view(torch.float8_e4m3fn).double().abs())).all())
    full = dy[:256].double() @ ext.dequantize_rows_fp8(wq, ws, N, K, torch.float32).double()
    rel = float((dx - full).norm() / full.norm())

    def fp8_arm():
        a, b = ext.quantize_rows_fp8_scaled(dy, ws)
        ext.fused_fp8_gemm_dx(a, b, wq, K)

    def materialize_arm():
        dy @ ext.dequantize_rows_fp8(wq, ws, N, K, BF)

    wd = ext.dequantize_rows_fp8(wq, ws, N, K, BF)
    variants = {
        "quantize_rows_fp8_scaled": lambda: ext.quantize_rows_fp8_scaled(dy, ws),
        "fused_fp8_gemm_dx": lambda: ext.fused_fp8_gemm_dx(gq, gs, wq, K),
        "dequantize_rows_fp8": lambda: ext.dequantize_rows_fp8(wq, ws, N, K, BF),
        "dy@w": lambda: dy @ wd,
        "fp8_arm": fp8_arm,
        "materialize_arm": materialize_arm,
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
    row["fp8_over_materialize"] = round(row["fp8_arm_us"] / row["materialize_arm_us"], 3)
    row["fused_fp8_gemm_dx_tflops"] = round(2.0 * M * N * K / row["fused_fp8_gemm_dx_us"] / 1e6, 1)
    row["dy@w_tflops"] = round(2.0 * M * N * K / row["dy@w_us"] / 1e6, 1)
    row["quantize_rows_fp8_scaled_gbs"] = round(
        3.0 * M * N / row["quantize_rows_fp8_scaled_us"] / 1e3, 1)
    return row


def model_steps(args):
    from relora_amd.models import build_model_from_config, load_model_config
    from relora_amd.ops.optim import AdamW
    from relora_amd.relora import ReLoRaModel

    cfg = load_model_config(args.model)
    runs = {}
    for on in (False, True):
        torch.manual_seed(0)
        model = ReLoRaModel(build_model_from_config(cfg), r=128, lora_alpha=32, lora_dropout=0.1,
                            target_modules=["attn", "attention", "mlp"],
                            keep_original_weights=True, quantize="fp8")
        model = model.to("cuda", dtype=BF).set_fp8_backward(on)
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        runs[on] = (model, opt)
    batch = torch.randint(0, cfg.vocab_size, (args.bs, args.seq), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(1))

    def steps(on, n):
        model, opt = runs[on]
        for _ in range(n):
            loss = model(input_ids=batch, labels=batch).loss
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        return float(loss)

    out = {on: {"ms": [], "peak_gib": 0.0} for on in runs}
    for on in runs:
        steps(on, args.warmup)
    for _ in range(args.rounds):          # alternate the two settings
        for on in runs:
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out[on]["loss"] = steps(on, args.steps)
            out[on]["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
            out[on]["peak_gib"] = max(out[on]["peak_gib"], torch.cuda.max_memory_allocated() / 2 ** 30)
    for on, o in out.items():
        ms = statistics.median(o["ms"])
        print(json.dumps({
            "model": args.model, "bs": args.bs, "seq": args.seq, "fp8_backward": on,
            "steps": args.warmup + args.rounds * args.steps, "loss": round(o["loss"], 4),
            "ms_per_step": round(ms, 1), "ms_spread": [round(min(o["ms"]), 1), round(max(o["ms"]), 1)],
            "tokens_per_s": round(args.bs * args.seq / ms * 1e3),
            "peak_gib_both_models_resident": round(o["peak_gib"], 2)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "model"])
    p.add_argument("--rounds", type=int, default=None)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--model", default="configs/llama_250m.json")
    p.add_argument("--bs", type=int, default=8)
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    if args.mode == "kernel":
        for M, N, K in SHAPES:
            print(json.dumps(bench_shape(M, N, K, args.rounds or 15, args.iters)), flush=True)
    else:
        args.rounds = args.rounds or 4
        model_steps(args)


if __name__ == "__main__":
    main()
