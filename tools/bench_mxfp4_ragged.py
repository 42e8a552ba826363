"""The MXFP4 arm for ragged widths on the MI355X against the materialize arm it replaces, at
llama_1b's MLP shapes (gate/up: N = 5461; down_proj: K = 5461).

  python tools/bench_mxfp4_ragged.py kernel [--N 5461 --K 2048] [--rounds 15] [--iters 20]
      quantize_rows_fp8(_padded) + fused_mxfp4_gemm_ragged  against  dequantize_rows_mxfp4 + F.linear +
      lora_add_nt_.  Arms alternate; the materialize arm is in the rotation twice, so the gap
      between its two medians is the spread of a run against itself.
  python tools/bench_mxfp4_ragged.py model [--model configs/llama_1b.json] [--bs 8] [--steps 5]
      ReLoRA training steps with quantize="mxfp4" on ONE model, the settings of (ragged N, ragged K)
      alternating, the one without the new arm (the parent commit's dispatch) twice: ms/step, tokens/s.
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
    x = torch.randn(M, K, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF)
    t, bw = (torch.randn(n, r, device="cuda", generator=g).to(BF) for n in (M, N))
    wq, ws = ext.quantize_rows_mxfp4(w)
    empty = x.new_empty(0)
    quantize = ext.quantize_rows_fp8_padded if K % 128 else ext.quantize_rows_fp8

    def fused():
        xq, xs = quantize(x)
        return ext.fused_mxfp4_gemm_ragged(xq, xs, wq, ws, N, K, t, bw, empty, 0.25)

    def materialize():
        y = F.linear(x, ext.dequantize_rows_mxfp4(wq, ws, N, K, BF))
        ext.lora_add_nt_(y, t, bw * 0.25)
        return y

    xq, xs = quantize(x)
    variants = {"fused": fused, "materialize": materialize, "materialize_again": materialize,
                "quantize": lambda: quantize(x),
                "gemm": lambda: ext.fused_mxfp4_gemm_ragged(xq, xs, wq, ws, N, K, t, bw, empty, 0.25)}
    # the two arms agree up to the e4m3 rounding of the activations
    a, b = fused()[:256].double(), materialize()[:256].double()
    row = {"M": M, "N": N, "K": K, "r": r, "rel_diff_fused_vs_materialize": round(float((a - b).norm() / b.norm()), 4)}
    for fn in variants.values():
        timed(fn, 5)
    samples = {k: [] for k in variants}
    for _ in range(args.rounds or 15):
        for k, fn in variants.items():
            samples[k].append(timed(fn, args.iters))
    for k, v in samples.items():
        row[k + "_us"] = [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]
    row["fused_over_materialize"] = round(row["fused_us"][0] / row["materialize_us"][0], 3)
    row["materialize_again_over_materialize"] = round(row["materialize_again_us"][0] / row["materialize_us"][0], 3)
    row["gemm_tflops"] = round(2.0 * M * N * K / row["gemm_us"][0] / 1e6, 1)
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
                      quantize="mxfp4").to("cuda", dtype=BF)
    opt = AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    batch = torch.randint(0, cfg.vocab_size, (args.bs, args.seq), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(1))
    # (label, ragged-N arm, ragged-K arm)
    settings = [("without", False, False), ("n", True, False), ("k", False, True), ("n_k", True, True),
                ("without_again", False, False)]

    def steps(n_on, k_on, n):
        Fn._MXFP4_RAGGED_N, Fn._MXFP4_RAGGED_K = n_on, k_on
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
                          "tokens_per_s": round(args.bs * args.seq / med * 1e3), "last_loss": round(loss, 4),
                          "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}),
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
