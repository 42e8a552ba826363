"""The fp8 arms for a ragged reduction width on the MI355X against the materialize arms they
replace, at llama_1b's down_proj shape (K = 5461).

  python tools/bench_fp8_kragged.py kernel [--rounds 15] [--iters 20]
      forward: quantize_rows_fp8_padded + fused_fp8_gemm_kragged  against  dequantize + F.linear +
      lora_add_nt_;  dx: quantize_rows_fp8_scaled_padded + fused_fp8_gemm_dx_kragged  against
      dequantize + dy @ w.  Arms alternate; each materialize arm is in the rotation twice, so the
      gap between its two medians is the spread of a run against itself.
  python tools/bench_fp8_kragged.py model [--model configs/llama_1b.json] [--bs 8] [--steps 5]
      ReLoRA training steps with quantize="fp8" on ONE model, the settings of (forward arm, dx arm,
      fp8_backward) alternating, the one without the new arms twice: ms/step and tokens/s.
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

from bench_fp8_ragged import BF, timed


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
        xq, xs = ext.quantize_rows_fp8_padded(x)
        return ext.fused_fp8_gemm_kragged(xq, xs, wq, ws, N, K, t, bw, empty, 0.25)

    def fwd_materialize():
        y = F.linear(x, ext.dequantize_rows_fp8(wq, ws, N, K, BF))
        ext.lora_add_nt_(y, t, bw * 0.25)
        return y

    def dx_fp8():
        gq, gs = ext.quantize_rows_fp8_scaled_padded(dy, ws)
        return ext.fused_fp8_gemm_dx_kragged(gq, gs, wq, N, K)

    def dx_materialize():
        return dy @ ext.dequantize_rows_fp8(wq, ws, N, K, BF)

    xq, xs = ext.quantize_rows_fp8_padded(x)
    gq, gs = ext.quantize_rows_fp8_scaled_padded(dy, ws)
    variants = {"fwd_fp8": fwd_fp8, "fwd_materialize": fwd_materialize, "dx_fp8": dx_fp8,
                "dx_materialize": dx_materialize, "fwd_materialize_again": fwd_materialize,
                "dx_materialize_again": dx_materialize,
                "quantize_rows_fp8_padded": lambda: ext.quantize_rows_fp8_padded(x),
                "fused_fp8_gemm_kragged": lambda: ext.fused_fp8_gemm_kragged(xq, xs, wq, ws, N, K, t, bw, empty, 0.25),
                "fused_fp8_gemm_dx_kragged": lambda: ext.fused_fp8_gemm_dx_kragged(gq, gs, wq, N, K)}
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
        row[p + "_materialize_again_over_materialize"] = round(
            row[p + "_materialize_again_us"][0] / row[p + "_materialize_us"][0], 3)
    for k in ("fused_fp8_gemm_kragged", "fused_fp8_gemm_dx_kragged"):
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
    # (label, forward arm, dx arm, fp8_backward)
    settings = [("without", False, False, False), ("fwd", True, False, False), ("without_again", False, False, False),
                ("bwd_without", False, False, True), ("bwd_fwd", True, False, True), ("bwd_fwd_dx", True, True, True),
                ("bwd_without_again", False, False, True)]

    def steps(fwd, dx, bwd, n):
        Fn._FP8_KRAGGED_FWD, Fn._FP8_KRAGGED_DX = fwd, dx
        net.set_fp8_backward(bwd)
        for _ in range(n):
            loss = net(input_ids=batch, labels=batch).loss
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        return float(loss.detach())

    ms = {s[0]: [] for s in settings}
    for s in settings:
        steps(*s[1:], args.warmup)
    for _ in range(args.rounds or 4):
        for s in settings:
            t0 = time.perf_counter()
            loss = steps(*s[1:], args.steps)
            ms[s[0]].append((time.perf_counter() - t0) / args.steps * 1e3)
    for label, v in ms.items():
        med = statistics.median(v)
        print(json.dumps({"model": args.model, "bs": args.bs, "seq": args.seq, "setting": label,
                          "ms_per_step": round(med, 1), "ms_spread": [round(min(v), 1), round(max(v), 1)],
                          "tokens_per_s": round(args.bs * args.seq / med * 1e3), "last_loss": round(loss, 4)}),
              flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "model"])
    p.add_argument("--rounds", type=int, default=None)
    p.add_argument("--iters", type=int, default=20)
    for n, v in (("M", 16384), ("N", 2048), ("K", 5461), ("r", 128), ("bs", 8), ("seq", 1024),
                 ("steps", 5), ("warmup", 3)):
        p.add_argument("--" + n, type=int, default=v)
    p.add_argument("--model", default="configs/llama_1b.json")
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    (kernel if args.mode == "kernel" else model)(args)


if __name__ == "__main__":
    main()
