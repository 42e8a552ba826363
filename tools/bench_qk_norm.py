"""Per-head QK RMSNorm + RoPE on the MI355X: kernel microbenchmark and a
feature-on training-step driver (bench.py has no switch for config.qk_norm).

  python tools/bench_qk_norm.py kernel [--B 8] [--nh 32] [--nkv 32] [--S 2048] [--hd 64]
      fused forward / backward (one launch each way, plus the dw fold) against
      the composition a user would otherwise run: ops.rmsnorm on the two
      [rows, hd] views plus ops.rope, and its autograd backward; and against
      the one-read-one-write HBM time of q and k.  The two sides alternate,
      --rounds times.
  python tools/bench_qk_norm.py model [--model configs/llama_1b.json] [--qk_norm true]
      the flagship ReLoRA step of bench.py with config.qk_norm set: ms/step
      and peak memory, one JSON line.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

HBM_BYTES_PER_S = 8.0e12  # MI355X peak; the achievable streaming rate is lower


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernel(args):
    from relora_amd import ops
    from relora_amd.ops import hip

    torch.manual_seed(0)
    B, nh, nkv, S, hd = args.B, args.nh, args.nkv or args.nh, args.S, args.hd
    dev, bf = "cuda", torch.bfloat16
    # the model's layout: transposed views of the projections' BSHD outputs
    qb = torch.randn(B, S, nh, hd, device=dev, dtype=bf)
    kb = torch.randn(B, S, nkv, hd, device=dev, dtype=bf)
    q, k = qb.transpose(1, 2), kb.transpose(1, 2)
    dqo, dko = torch.randn_like(q), torch.randn_like(k)
    wq = (1 + 0.1 * torch.randn(hd, device=dev)).to(bf)
    wk = (1 + 0.1 * torch.randn(hd, device=dev)).to(bf)
    cos, sin = (t.to(dev) for t in ops.build_rope_cache(hd, S))
    ext = hip.ext()

    qo, ko, iq, ik = ext.qk_norm_rope_fwd(q, k, wq, wk, cos, sin, 1e-6)

    def fused_fwd():
        ext.qk_norm_rope_fwd(q, k, wq, wk, cos, sin, 1e-6)

    def fused_bwd():
        ext.qk_norm_rope_bwd(dqo, dko, q, k, wq, wk, iq, ik, cos, sin)

    # the composition, kernel for kernel (what ops.rmsnorm + ops.rope launch)
    q2, k2 = qb.view(-1, hd), kb.view(-1, hd)
    nq, inv_q = ext.rmsnorm_fwd(q2, wq, 1e-6)
    nk, inv_k = ext.rmsnorm_fwd(k2, wk, 1e-6)
    nq4 = nq.view(B, S, nh, hd).transpose(1, 2)
    nk4 = nk.view(B, S, nkv, hd).transpose(1, 2)

    def comp_fwd():
        a, _ = ext.rmsnorm_fwd(q2, wq, 1e-6)
        b, _ = ext.rmsnorm_fwd(k2, wk, 1e-6)
        ext.rope_fwd(a.view(B, S, nh, hd).transpose(1, 2),
                     b.view(B, S, nkv, hd).transpose(1, 2), cos, sin, False)

    def comp_bwd():
        da, db = ext.rope_fwd(dqo, dko, cos, sin, True)
        ext.rmsnorm_bwd(q2, wq, inv_q, da.transpose(1, 2).reshape(-1, hd))
        ext.rmsnorm_bwd(k2, wk, inv_k, db.transpose(1, 2).reshape(-1, hd))

    # both sides compute the same thing: the row sums are added in another
    # order, so a rare element may round to the neighbouring bf16
    ref = ext.rope_fwd(nq4, nk4, cos, sin, False)
    for a, b in ((ref[0], qo), (ref[1], ko)):
        assert (a.float() - b.float()).abs().max() <= 2.0 ** -7 * a.float().abs().max()

    elems = (q.numel() + k.numel())
    floor_fwd = 2 * elems * 2 / HBM_BYTES_PER_S * 1e6       # read x, write out
    floor_bwd = 3 * elems * 2 / HBM_BYTES_PER_S * 1e6       # read x and dy, write dx
    res = {"fused_fwd": [], "comp_fwd": [], "fused_bwd": [], "comp_bwd": []}
    for _ in range(args.rounds):
        for name, fn in (("fused_fwd", fused_fwd), ("comp_fwd", comp_fwd),
                         ("fused_bwd", fused_bwd), ("comp_bwd", comp_bwd)):
            res[name].append(_time(fn, args.iters, args.warmup))
    out = {"shape": [B, nh, nkv, S, hd], "iters": args.iters, "rounds": args.rounds,
           "hbm_floor_us": {"fwd": round(floor_fwd, 1), "bwd": round(floor_bwd, 1)}}
    for name, v in res.items():
        out[name + "_us"] = {"min": round(min(v), 1), "max": round(max(v), 1),
                             "median": round(sorted(v)[len(v) // 2], 1)}
    for d in ("fwd", "bwd"):
        out[f"speedup_{d}"] = round(out[f"comp_{d}_us"]["median"]
                                    / out[f"fused_{d}_us"]["median"], 2)
    print(json.dumps(out))


def model(args):
    from relora_amd.models import build_model_from_config, load_model_config
    from relora_amd.ops.optim import AdamW, clip_grad_norm_
    from relora_amd.ops.tunable import enable_tuned_gemms
    from relora_amd.relora import ReLoRaModel

    torch.manual_seed(1234)
    enable_tuned_gemms()
    cfg = load_model_config(args.model)
    cfg.qk_norm = args.qk_norm
    net = build_model_from_config(cfg)
    net = ReLoRaModel(net, r=args.lora_r, lora_alpha=32, lora_dropout=0.1,
                      target_modules=["attn", "attention", "mlp"], keep_original_weights=True)
    net = net.to(device="cuda", dtype=torch.bfloat16).train()
    trainable = [p for p in net.parameters() if p.requires_grad]
    opt = AdamW(trainable, lr=4e-4, betas=(0.9, 0.95), weight_decay=0.01)
    g = torch.Generator().manual_seed(42)
    batches = [torch.randint(0, cfg.vocab_size, (args.batch_size, args.seq_len), generator=g).cuda()
               for _ in range(args.warmup + args.steps)]

    def step(batch):
        loss = net(input_ids=batch, labels=batch).loss
        loss.backward()
        clip_grad_norm_(trainable, 1.0, error_if_nonfinite=True)
        opt.step()
        for prm in trainable:
            prm.grad = None
        return loss

    for i in range(args.warmup):
        step(batches[i])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(batches[args.warmup + i])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps({
        "model": args.model, "qk_norm": bool(args.qk_norm), "ms_per_step": round(ms, 2),
        "tokens_per_s": round(args.batch_size * args.seq_len / ms * 1e3),
        "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3),
        "loss": round(loss.item(), 4), "steps": args.steps}))


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("kernel")
    a.add_argument("--B", type=int, default=8)
    a.add_argument("--nh", type=int, default=32)
    a.add_argument("--nkv", type=int, default=None)
    a.add_argument("--S", type=int, default=2048)
    a.add_argument("--hd", type=int, default=64)
    a.add_argument("--iters", type=int, default=50)
    a.add_argument("--warmup", type=int, default=5)
    a.add_argument("--rounds", type=int, default=5)
    b = sub.add_parser("model")
    b.add_argument("--model", type=str, default="configs/llama_1b.json")
    b.add_argument("--qk_norm", type=lambda x: x.lower() == "true", default=True)
    b.add_argument("--batch_size", type=int, default=8)
    b.add_argument("--seq_len", type=int, default=2048)
    b.add_argument("--lora_r", type=int, default=128)
    b.add_argument("--steps", type=int, default=20)
    b.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm.py measures on a GPU; none is available")
    kernel(args) if args.cmd == "kernel" else model(args)


if __name__ == "__main__":
    main()
