"""Child-process worker for tests/test_gpu_lora_group.py.

RELORA_AMD_LORA_GROUP is read once at import, so grouping on and off each
need a fresh process.  `python tests/lora_group_worker.py OUT.pt` builds a
2-layer llama (hidden 64, intermediate 171 — odd, like the flagship's 5461 —
2 heads, r 32), runs one forward/backward at seq 64, bs 2 and then 3 AdamW
steps under whatever environment it was started with, counts entries into the
group op, and saves {entered, loss, grads, losses} to OUT.pt.
"""

import os
import sys

import torch


def main(out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from relora_amd import ops
    from relora_amd.models import LlamaConfig, build_model_from_config
    from relora_amd.ops.functional import set_dropout_rng_state
    from relora_amd.relora import ReLoRaModel

    assert torch.cuda.is_available(), "lora group worker needs a GPU"
    entered = [0]
    real = ops.lora_linear_group

    def counting(*a, **kw):
        entered[0] += 1
        return real(*a, **kw)

    ops.lora_linear_group = counting

    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=256, hidden_size=64, intermediate_size=171,
                      num_hidden_layers=2, num_attention_heads=2,
                      max_position_embeddings=64)
    model = build_model_from_config(cfg)
    model = ReLoRaModel(model, r=32, lora_alpha=32, lora_dropout=0.1,
                        target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True)
    with torch.no_grad():  # lora_B starts at zero: give the LoRA path a signal
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.normal_(std=0.05)
    model = model.to(device="cuda", dtype=torch.bfloat16)
    model.train()
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, cfg.vocab_size, (2, 64), generator=g).cuda()

    set_dropout_rng_state(0)
    loss = model(input_ids=x, labels=x).loss
    loss.backward()
    grads = {n: p.grad.detach().float().cpu()
             for n, p in model.named_parameters() if p.requires_grad}
    first_loss = float(loss)

    trainable = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(trainable, lr=1e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model(input_ids=x, labels=x).loss
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        losses.append(float(model(input_ids=x, labels=x).loss))
    torch.cuda.synchronize()
    torch.save({"entered": entered[0], "loss": first_loss, "grads": grads,
                "losses": losses}, out_path)
    print("LORA_GROUP_WORKER_DONE", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
