"""Record the golden vectors that tests/test_reference_parity.py compares
against (tests/golden/reference_parity/).

The parity tests used to import the reference implementation at test time;
this tool does that import ONCE, runs the reference on small fixed cases and
stores what it was given and what it returned, so the suite itself needs
nothing outside the repository.  Re-run it only when a case changes:

  python tools/record_reference_golden.py --reference /path/to/relora

Only data is written (weights, inputs, outputs, checkpoints the reference
saved) — never any of the reference's code.
"""

import argparse
import importlib.machinery
import json
import logging
import os
import shutil
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "reference_parity")

LLAMA_KW = dict(vocab_size=128, hidden_size=64, intermediate_size=172,
                num_hidden_layers=2, num_attention_heads=4,
                max_position_embeddings=64, rms_norm_eps=1e-6,
                pad_token_id=None, bos_token_id=0, eos_token_id=1)
RELORA_KW = dict(r=8, lora_alpha=32, lora_dropout=0.0,
                 target_modules=["attn", "attention", "mlp"],
                 keep_original_weights=True)


def _stub(name, **attrs):
    """Minimal stand-in for a reference-only dependency the recorded code
    paths never touch (bitsandbytes/wandb/loguru)."""
    if name in sys.modules:
        return sys.modules[name]
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, loader=None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _np(t):
    # a copy: several recorded tensors are modified in place afterwards
    return t.detach().cpu().numpy().copy()


def _sd(model, drop=("rotary_emb.inv_freq",)):
    return {k: v.clone() for k, v in model.state_dict().items()
            if not any(d in k for d in drop)}


def _save(name, **arrays):
    np.savez_compressed(os.path.join(OUT, name), **arrays)


def record_llama(ref_llama):
    from transformers import LlamaConfig as HFLlamaConfig
    torch.manual_seed(0)
    ref = ref_llama.LlamaForCausalLM(HFLlamaConfig(**LLAMA_KW))
    x = torch.randint(0, 128, (2, 32))
    with torch.no_grad():
        logits = ref(input_ids=x).logits
    out = ref(input_ids=x, labels=x)
    out.loss.backward()
    arrays = {f"w/{k}": _np(v) for k, v in _sd(ref).items()}
    arrays.update({f"g/{n}": _np(p.grad) for n, p in ref.named_parameters()})
    _save("llama_fwd_bwd.npz", x=_np(x), logits=_np(logits),
          loss=_np(out.loss), **arrays)


def record_relora(ref_llama, ref_relora):
    from transformers import LlamaConfig as HFLlamaConfig
    torch.manual_seed(1)
    base = ref_llama.LlamaForCausalLM(HFLlamaConfig(**LLAMA_KW))
    arrays = {f"w/{k}": _np(v) for k, v in _sd(base).items()}
    wrapped = ref_relora.ReLoRaModel(base, **RELORA_KW)
    torch.manual_seed(2)
    with torch.no_grad():
        for n, p in sorted((n, p) for n, p in wrapped.named_parameters()
                           if "lora_" in n):
            p.copy_(torch.randn_like(p) * 0.05)
            arrays[f"lora/{n}"] = _np(p)
    x = torch.randint(0, 128, (2, 24))
    wrapped.eval()
    with torch.no_grad():
        loss = wrapped(input_ids=x, labels=x).loss
    wrapped.merge_and_reinit()
    arrays.update({f"merged/{n}": _np(p) for n, p in wrapped.named_parameters()
                   if "lora_" not in n})
    _save("relora_merge.npz", x=_np(x), loss=_np(loss), **arrays)


def record_scheduler(ref_tu):
    cases = []
    for kwargs in (
        dict(num_training_steps=120, warmup_steps=10, min_lr_ratio=0.1,
             cycle_length=40, restart_warmup_steps=5, adjust_step=0),
        dict(num_training_steps=240, warmup_steps=10, min_lr_ratio=0.2,
             cycle_length=60, restart_warmup_steps=10, adjust_step=40),
    ):
        p = torch.nn.Parameter(torch.zeros(1))
        o = torch.optim.SGD([p], lr=1.0)
        s = ref_tu.get_scheculer(optimizer=o, scheduler_type="cosine_restarts",
                                 **kwargs)
        lrs = []
        for _ in range(kwargs["num_training_steps"]):
            lrs.append(float(o.param_groups[0]["lr"]))
            o.step()
            s.step()
        cases.append({"kwargs": kwargs, "lrs": lrs})
    with open(os.path.join(OUT, "scheduler.json"), "w") as f:
        # repr round-trips a double exactly
        json.dump(cases, f, indent=0)


def record_pythia(ref_pythia):
    from transformers import GPTNeoXConfig as HFNeoXConfig
    kw = dict(vocab_size=128, hidden_size=64, num_hidden_layers=2,
              num_attention_heads=4, intermediate_size=256,
              max_position_embeddings=64, rotary_pct=0.25,
              use_parallel_residual=True, tie_word_embeddings=False,
              layer_norm_eps=1e-5)
    torch.manual_seed(4)
    hf_cfg = HFNeoXConfig(**{k: v for k, v in kw.items() if k != "rotary_pct"})
    # the reference model was written against an older transformers config
    # surface; restore the legacy attribute names it reads
    hf_cfg.rotary_pct = kw["rotary_pct"]
    hf_cfg.rotary_emb_base = 10000
    hf_cfg.rope_scaling = None
    hf_cfg.attention_dropout = 0.0
    hf_cfg.hidden_dropout = 0.0
    ref = ref_pythia.GPTNeoXForCausalLM(hf_cfg)
    ref.gpt_neox.get_head_mask = lambda head_mask, n: [None] * n
    arrays = {f"w/{k}": _np(v) for k, v in _sd(
        ref, drop=("rotary_emb.inv_freq", "attention.bias", "masked_bias")).items()}

    torch.manual_seed(9)
    x = torch.randint(0, 128, (2, 32))
    # explicit all-ones mask: routes the reference through its causal branch
    # (its eval-mode B>1 path without a mask is non-causal)
    am = torch.ones_like(x)
    ref.eval()
    with torch.no_grad():
        logits = ref(input_ids=x, attention_mask=am).logits
    loss_eval = ref(input_ids=x, attention_mask=am, labels=x).loss
    ref.train()
    loss_train = ref(input_ids=x, labels=x).loss
    loss_train.backward()
    nograd = []
    for n, p in ref.named_parameters():
        if p.grad is None:
            nograd.append(n)
        else:
            arrays[f"g/{n}"] = _np(p.grad)
    _save("pythia_fwd_bwd.npz", x=_np(x), logits=_np(logits),
          loss_eval=_np(loss_eval), loss_train=_np(loss_train),
          nograd=np.array(nograd, dtype=str), **arrays)


def record_optimizer_reset(ref_tu):
    torch.manual_seed(5)
    t = torch.randn(1000)
    t_pruned = t.clone()
    ref_tu.magnitude_pruning_(t_pruned, 0.7)
    arrays = dict(t=_np(t), t_pruned=_np(t_pruned))

    torch.manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(64, 32)) for _ in range(3)]
    opt = torch.optim.Adam(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()
    for i, p in enumerate(ps):
        arrays[f"p/{i}"] = _np(p)
        for k in ("exp_avg", "exp_avg_sq"):
            arrays[f"before/{k}/{i}"] = _np(opt.state[p][k]).copy()
    ref_tu.optimizer_reset(opt, reset_params=ps[:2],
                           optimizer_state_keys=["exp_avg", "exp_avg_sq"],
                           reset_optimizer_on_relora=False,
                           optimizer_random_pruning=0.0,
                           optimizer_magnitude_pruning=0.9)
    for i, p in enumerate(ps):
        for k in ("exp_avg", "exp_avg_sq"):
            arrays[f"after/{k}/{i}"] = _np(opt.state[p][k])
    _save("optimizer_reset.npz", **arrays)


def make_tokenizer_and_texts():
    """A 40-word WordLevel tokenizer (the test builds the same one) and 60
    texts (stored, so the test reads them back)."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    words = [f"w{i}" for i in range(40)]
    vocab = {"[PAD]": 0, "[UNK]": 1, "</s>": 2}
    for w in words:
        vocab[w] = len(vocab)
    tok = Tokenizer(models.WordLevel(vocab=vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="[PAD]",
                                   unk_token="[UNK]", eos_token="</s>")
    rng = np.random.RandomState(3)
    texts = [" ".join(rng.choice(words, size=rng.randint(3, 30)))
             for _ in range(60)]
    return fast, texts


def record_tokenize(ref_dl):
    import datasets as hfds
    fast, texts = make_tokenizer_and_texts()
    ds = hfds.DatasetDict({"train": hfds.Dataset.from_dict({"text": list(texts)})})
    out = ref_dl.tokenize_and_chunk(fast, ds, "text", 16, num_cpu=1)["train"]
    with open(os.path.join(OUT, "tokenize_and_chunk.json"), "w") as f:
        json.dump({"texts": texts,
                   "column_names": sorted(out.column_names),
                   "input_ids": [out[i]["input_ids"] for i in range(len(out))]},
                  f)


def record_checkpoints(ref_llama, ref_relora):
    from transformers import LlamaConfig as HFLlamaConfig

    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaForCausalLM as OurLlama
    from relora_amd.relora import ReLoRaModel as OurReLoRa

    torch.manual_seed(11)
    base = ref_llama.LlamaForCausalLM(HFLlamaConfig(**LLAMA_KW))
    ref_wrapped = ref_relora.ReLoRaModel(base, **RELORA_KW)
    with torch.no_grad():
        for n, p in ref_wrapped.named_parameters():
            if "lora_" in n:
                p.copy_(torch.randn_like(p) * 0.03)
    ref_dir = os.path.join(OUT, "ckpt_written_by_reference")
    shutil.rmtree(ref_dir, ignore_errors=True)
    ref_wrapped.save_pretrained(ref_dir)

    x = torch.randint(0, 128, (2, 16))
    ref_wrapped.eval()
    with torch.no_grad():
        loss_ref = ref_wrapped(input_ids=x, labels=x).loss

    # ours -> reference: the checkpoint OUR save_pretrained wrote, and the
    # loss the reference computed after loading it
    torch.manual_seed(12)
    our_wrapped = OurReLoRa(OurLlama(LlamaConfig(**LLAMA_KW)), **RELORA_KW)
    with torch.no_grad():
        for n, p in our_wrapped.named_parameters():
            if "lora_" in n:
                p.copy_(torch.randn_like(p) * 0.03)
    our_dir = os.path.join(OUT, "ckpt_read_by_reference")
    shutil.rmtree(our_dir, ignore_errors=True)
    our_wrapped.save_pretrained(our_dir)
    ref_loaded = ref_relora.ReLoRaModel.from_pretrained(our_dir)
    ref_loaded.eval()
    with torch.no_grad():
        loss_ref_loaded = ref_loaded(input_ids=x, labels=x).loss
    _save("checkpoint_losses.npz", x=_np(x), loss_ref=_np(loss_ref),
          loss_ref_loaded=_np(loss_ref_loaded))


def record_megatron(ref_ds):
    rng = np.random.RandomState(0)
    arrays = {}
    for trial in range(5):
        n_docs = int(rng.randint(2, 50))
        sizes = rng.randint(1, 60, size=n_docs).astype(np.int32)
        seq_length = int(rng.randint(2, 33))
        num_epochs = int(rng.randint(1, 4))
        seed = int(rng.randint(0, 10000))
        documents = np.arange(n_docs, dtype=np.int32)
        doc_idx = ref_ds._build_doc_idx(documents, num_epochs,
                                        np.random.RandomState(seed))
        sample_idx = ref_ds._build_sample_idx(sizes, doc_idx, seq_length,
                                              num_epochs, int(sizes.sum()))
        shuffle_idx = ref_ds._build_shuffle_idx(sample_idx.shape[0] - 1,
                                                np.random.RandomState(seed + 1))
        arrays[f"{trial}/sizes"] = sizes
        arrays[f"{trial}/params"] = np.array([seq_length, num_epochs, seed])
        arrays[f"{trial}/doc_idx"] = doc_idx
        arrays[f"{trial}/sample_idx"] = sample_idx
        arrays[f"{trial}/shuffle_idx"] = shuffle_idx
    _save("megatron_index.npz", **arrays)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reference", required=True,
                    help="checkout of the reference implementation")
    args = ap.parse_args()

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(args.reference))
    _stub("bitsandbytes", functional=_stub("bitsandbytes.functional"))
    _stub("wandb", AlertLevel=type("AlertLevel", (), {"WARN": "WARN"}),
          alert=lambda **kw: None)
    _stub("loguru", logger=logging.getLogger("ref"))
    from peft_pretraining import dataloader as ref_dl
    from peft_pretraining import modeling_llama as ref_llama
    from peft_pretraining import modeling_pythia as ref_pythia
    from peft_pretraining import relora as ref_relora
    from peft_pretraining import training_utils as ref_tu
    from peft_pretraining.megatron_dataset import dataset as ref_ds

    os.makedirs(OUT, exist_ok=True)
    record_llama(ref_llama)
    record_relora(ref_llama, ref_relora)
    record_scheduler(ref_tu)
    record_pythia(ref_pythia)
    record_optimizer_reset(ref_tu)
    record_tokenize(ref_dl)
    record_checkpoints(ref_llama, ref_relora)
    record_megatron(ref_ds)
    print(f"golden vectors written to {OUT}")


if __name__ == "__main__":
    main()
