"""The ragged-width fp8 arms on the MI355X against the materialize arms they replace, at
llama_1b's gate/up shape (N = 5461).

  python tools/bench_fp8_ragged.py kernel [--rounds 15] [--iters 20]
      forward: quantize_rows_fp8 + fused_fp8_gemm_ragged  against  dequantize + F.linear +
      lora_add_nt_;  dx: quantize_rows_fp8_scaled_padded + fused_fp8_gemm_dx_ragged  against
      dequantize + dy @ w.  Arms alternate; medians with min/max over the rounds.
  python tools/bench_fp8_ragged.py model [--model configs/llama_1b.json] [--bs 8] [--steps 5]
      ReLoRA training steps with quantize="fp8" on ONE model, the four settings of
      (RELORA_AMD_FP8_RAGGED, fp8_backward) alternating: ms/step and tokens/s.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch
import torch.nn.functional as F

BF = torch.bfloat16


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernel(args):
    from relora_amd.ops import hip
    ext = hip.ext_or_raise()
    M, N, K, r = args.M, args.N, args.K, args.r
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x, dy = (torch.randn(M, n, device="cuda", generator=g).to(BF) for n in (K, N))
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    t, bw = (torch.randn(n, r, device="cuda", generator=g).to(BF) for n in (M, N))
    wq, ws = ext.quantize_rows_fp8(w)
    empty = x.new_empty(0)

    def fwd_fp8():
        xq, xs = ext.quantize_rows_fp8(x)
        return ext.fused_fp8_gemm_ragged(xq, xs, wq, ws, N, t, bw, empty, 0.25)

    def fwd_materialize():
        y = F.linear(x, ext.dequantize_rows_fp8(wq, ws, N, K, BF))
        ext.lora_add_nt_(y, t, bw * 0.25)
        return y

    def dx_fp8():
        gq, gs = ext.quantize_rows_fp8_scaled_padded(dy, ws)
        return ext.fused_fp8_gemm_dx_ragged(gq, gs, wq, N, K)

    def dx_materialize():
        return dy @ ext.dequantize_rows_fp8(wq, ws, N, K, BF)

    xq, xs = ext.quantize_rows_fp8(x)
    gq, gs = ext.quantize_rows_fp8_scaled_padded(dy, ws)
    variants = {"fwd_fp8": fwd_fp8, "fwd_materialize": fwd_materialize, "dx_fp8": dx_fp8,
                "dx_materialize": dx_materialize,
                "fused_fp8_gemm_ragged": lambda: ext.fused_fp8_gemm_ragged(xq, xs, wq, ws, N, t, bw, empty, 0.25),
                "fused_fp8_gemm_dx_ragged": lambda: ext.fused_fp8_gemm_dx_ragged(gq, gs, wq, N, K),
                "quantize_rows_fp8_scaled_padded": lambda: ext.quantize_rows_fp8_scaled_padded(dy, ws)}
    # the two arms agree up to the e4m3 rounding of the activations / the gradient
    rel = {k: float((a()[:256].double() - b()[:256].double()).norm() / b()[:256].double().norm())
           for k, a, b in (("fwd", fwd_fp8, fwd_materialize), ("dx", dx_fp8, dx_materialize))}
    for fn in variants.values():
        timed(fn, 5)
    samples = {k: [] for k in variants}
    for _ in range(args.rounds or 15):
        for k, fn in variants.items():
            samples[k].append(timed(fn, args.iters))
    row = {"M": M, "N": N, "K": K, "r": r, "rel_diff_fp8_vs_materialize": {k: round(v, 4) for k, v in rel.items()}}
    for k, v in samples.items():
        row[k + "_us"] = [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
    for p in ("fwd", "dx"):
        row[p + "_fp8_over_materialize"] = round(row[p + "_fp8_us"][0] / row[p + "_materialize_us"][0], 3)
    for k in ("fused_fp8_gemm_ragged", "fused_fp8_gemm_dx_ragged"):
        row[k + "_tflops"] = round(2.0 * M * N * K / row[k + "_us"][0] / 1e6, 1)
    print(json.dumps(row), flush=True)


def model(args):
    import relora_amd.ops.functional as Fn
    from relora_amd.models import build_model_from_config, load_model_config
    from relora_amd.ops.optim import AdamW
    from relora_amd.relora import ReLoRaModel

    cfg = load_model_config(args.model)
    torch.manual_seed(0)
    net = ReLoRaModel(build_model_from_config(cfg), r=128, lora_alpha=32, lora_dropout=0.1,
                      target_modules=["attn", "attention", "mlp"], keep_original_weights=True,
                      quantize="fp8").to("cuda", dtype=BF)
    opt = AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    batch = torch.randint(0, cfg.vocab_size, (args.bs, args.seq), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(1))
    settings = [(rag, bwd) for bwd in (False, True) for rag in (False, True)]

    def steps(rag, bwd, n):
        Fn._FP8_RAGGED = rag
        net.set_fp8_backward(bwd)
        for _ in range(n):
            loss = net(input_ids=batch, labels=batch).loss
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        return float(loss.detach())

    ms = {s: [] for s in settings}
    for s in settings:
        steps(*s, args.warmup)
    for _ in range(args.rounds or 4):
        for s in settings:
            t0 = time.perf_counter()
            loss = steps(*s, args.steps)
            ms[s].append((time.perf_counter() - t0) / args.steps * 1e3)
    for (rag, bwd), v in ms.items():
        med = statistics.median(v)
        print(json.dumps({"model": args.model, "bs": args.bs, "seq": args.seq, "fp8_ragged": rag,
                          "fp8_backward": bwd, "ms_per_step": round(med, 1),
                          "ms_spread": [round(min(v), 1), round(max(v), 1)],
                          "tokens_per_s": round(args.bs * args.seq / med * 1e3), "last_loss": round(loss, 4)}),
              flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "model"])
    p.add_argument("--rounds", type=int, default=None)
    p.add_argument("--iters", type=int, default=20)
    for n, v in (("M", 16384), ("N", 5461), ("K", 2048), ("r", 128), ("bs", 8), ("seq", 1024),
                 ("steps", 5), ("warmup", 3)):
        p.add_argument("--" + n, type=int, default=v)
    p.add_argument("--model", default="configs/llama_1b.json")
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    (kernel if args.mode == "kernel" else model)(args)


if __name__ == "__main__":
    main()
