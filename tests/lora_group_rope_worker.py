"""Child-process worker for tests/test_gpu_lora_group_rope.py.

RELORA_AMD_LORA_GROUP_ROPE is read once at import, so the rotation in the
group's LoRA epilogue on and off each need a fresh process.  `python
tests/lora_group_rope_worker.py OUT.pt` runs, under whatever environment it was
started with,
  * lora_group_forward(x, mods, rope=...) forward and backward for every case
    of CASES, in training mode (dropout p = 0.1) and in eval mode, and
  * a 2-layer ReLoRA LLaMA (hidden 256, 4 heads; also 2 kv heads) forward and
    backward,
and saves {switch, cases, eval, llama, fused_calls} to OUT.pt.  fused_calls
counts, per case, the group-op calls that were asked to rotate (each is one
lora_add_nt_rope_group_ launch).

The test module imports CASES, make_modules and make_io from here, so both
sides build the same inputs.
"""

import os
import sys

import torch

B, S, K = 2, 96, 256
CASES = {
    # name: (head_dim, Ns, r, flags)
    "hd64_gqa": (64, (256, 128, 128), 32, (True, True, False)),
    "hd64_r128": (64, (256, 256, 256), 128, (True, True, False)),
    "hd128": (128, (256, 256, 256), 32, (True, True, False)),
    "g2": (64, (256, 128), 32, (True, False)),
    "hd96_fallback": (96, (192, 192, 192), 32, (True, True, False)),
}
P, C0, TORCH_SEED = 0.1, 1000, 11


def make_modules(Ns, r, train=True):
    from relora_amd.relora import ReLoRaLinear

    torch.manual_seed(31)
    mods = []
    for N in Ns:
        m = ReLoRaLinear(K, N, r=r, lora_alpha=16, lora_dropout=P, bias=False)
        with torch.no_grad():
            m.weight.normal_(std=0.05)
            m.lora_A.weight.normal_(std=0.05)
            m.lora_B.weight.normal_(std=0.05)
        m = m.to(device="cuda", dtype=torch.bfloat16)
        mods.append(m.train() if train else m.eval())
    return mods


def make_io(Ns, hd, seed=21):
    from relora_amd import ops

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, K, generator=g).to(torch.bfloat16).cuda()
    dys = [torch.randn(B, S, N, generator=g).to(torch.bfloat16).cuda() for N in Ns]
    cos, sin = ops.build_rope_cache(hd, 128, device="cuda")  # longer than S
    return x, dys, cos, sin


def run_case(name, train, counter):
    from relora_amd.ops.functional import set_dropout_rng_state
    from relora_amd.relora import lora_group_forward

    hd, Ns, r, flags = CASES[name]
    mods = make_modules(Ns, r, train)
    x, dys, cos, sin = make_io(Ns, hd)
    x.requires_grad_(True)
    set_dropout_rng_state(C0)
    del counter[:]
    ys = lora_group_forward(x, mods, rope=(cos, sin, flags, hd))
    fused = len(counter)
    torch.autograd.backward(ys, dys)
    return {
        "ys": [y.detach().cpu() for y in ys],
        "dx": x.grad.cpu(),
        "dAs": [m.lora_A.weight.grad.cpu() for m in mods],
        "dBs": [m.lora_B.weight.grad.cpu() for m in mods],
    }, fused


def run_llama(nkv):
    from relora_amd.models import build_model_from_config
    from relora_amd.models.config import LlamaConfig
    from relora_amd.ops.functional import set_dropout_rng_state
    from relora_amd.relora import ReLoRaModel

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=128, hidden_size=256, intermediate_size=344,
                      num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=nkv,
                      max_position_embeddings=128)
    model = ReLoRaModel(build_model_from_config(cfg), r=32, lora_alpha=32, lora_dropout=0.1,
                        target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True)
    model = model.to(device="cuda", dtype=torch.bfloat16).train()
    with torch.no_grad():  # lora_B starts at zero: make the LoRA path count
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.normal_(std=0.05)
    ids = torch.randint(0, 128, (B, S), generator=torch.Generator().manual_seed(1)).cuda()
    set_dropout_rng_state(C0)
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    gq = [p.grad for n, p in model.named_parameters() if "q_proj.lora_A" in n][0]
    return {"loss": loss.detach().float().cpu(), "dA_q0": gq.cpu()}


def main(out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd import ops
    from relora_amd.ops import functional as Fn

    assert torch.cuda.is_available(), "lora group rope worker needs a GPU"
    counter = []
    real = ops.lora_linear_group

    def counting(*a, **kw):
        if kw.get("rope") is not None:
            counter.append(1)
        return real(*a, **kw)

    ops.lora_linear_group = counting
    torch.manual_seed(TORCH_SEED)
    res = {"switch": Fn._LORA_GROUP_ROPE, "cases": {}, "eval": {}, "fused_calls": {},
           "llama": {}}
    for name in CASES:
        res["cases"][name], res["fused_calls"][name] = run_case(name, True, counter)
        res["eval"][name], _ = run_case(name, False, counter)
    del counter[:]
    for nkv in (4, 2):
        res["llama"][nkv] = run_llama(nkv)
    res["fused_calls"]["llama"] = len(counter)
    torch.cuda.synchronize()
    torch.save(res, out_path)
    print("LORA_GROUP_ROPE_WORKER_DONE", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
