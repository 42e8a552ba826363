"""Numerical parity against the ACTUAL reference implementation: same config
+ same weights -> same loss, logits and gradients on CPU fp32.

The reference is not imported here.  tools/record_reference_golden.py ran it
once on the cases below and stored what it was given (weights, inputs) and
what it returned under tests/golden/reference_parity/; each test feeds the
same weights and inputs to our implementation and compares with the recorded
reference results at the tolerance the live comparison used."""

import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "reference_parity")

LLAMA_KW = dict(vocab_size=128, hidden_size=64, intermediate_size=172,
                num_hidden_layers=2, num_attention_heads=4,
                max_position_embeddings=64, rms_norm_eps=1e-6,
                pad_token_id=None, bos_token_id=0, eos_token_id=1)
RELORA_KW = dict(r=8, lora_alpha=32, lora_dropout=0.0,
                 target_modules=["attn", "attention", "mlp"],
                 keep_original_weights=True)


def _load(name):
    """npz -> {key: tensor}; keys are '<group>/<name>' or plain names."""
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: (z[k] if z[k].dtype.kind == "U" else torch.from_numpy(z[k]))
                for k in z.files}


def _group(d, prefix):
    return {k[len(prefix) + 1:]: v for k, v in d.items()
            if k.startswith(prefix + "/")}


def _our_llama():
    from relora_amd.models.config import LlamaConfig
    from relora_amd.models.llama import LlamaForCausalLM
    return LlamaForCausalLM(LlamaConfig(**LLAMA_KW))


def test_llama_forward_backward_matches_reference():
    g = _load("llama_fwd_bwd.npz")
    ours = _our_llama()

    # port weights by name (architectures line up 1:1 modulo the reference's
    # persistent rotary inv_freq buffers — ours are non-persistent fp32 caches)
    ref_sd = _group(g, "w")
    our_sd = ours.state_dict()
    assert set(ref_sd) == set(our_sd), (set(ref_sd) ^ set(our_sd))
    ours.load_state_dict(ref_sd)

    x = g["x"]
    # logits: label-free forward (our fused-CE path returns logits=None when
    # labels are given, by design — it never materializes them)
    with torch.no_grad():
        ol = ours(input_ids=x).logits
    assert torch.allclose(g["logits"], ol, atol=1e-5), (g["logits"] - ol).abs().max()

    our_out = ours(input_ids=x, labels=x)
    assert torch.allclose(g["loss"], our_out.loss, atol=1e-6), \
        (g["loss"], our_out.loss)

    our_out.loss.backward()
    ref_grads = _group(g, "g")
    for (n, gr), (_, po) in zip(sorted(ref_grads.items()),
                                sorted(ours.named_parameters())):
        assert torch.allclose(gr, po.grad, atol=1e-5), n


def test_relora_wrap_and_merge_match_reference():
    from relora_amd.relora import ReLoRaModel as OurReLoRa

    g = _load("relora_merge.npz")
    ours_base = _our_llama()
    ours_base.load_state_dict(_group(g, "w"))
    our_wrapped = OurReLoRa(ours_base, **RELORA_KW)

    # the lora weights the reference ran with, paired by sorted name
    ref_lora = sorted(_group(g, "lora").items())
    our_lora = sorted((n, p) for n, p in our_wrapped.named_parameters()
                      if "lora_" in n)
    assert len(ref_lora) == len(our_lora)
    with torch.no_grad():
        for (rn, val), (on, op) in zip(ref_lora, our_lora):
            op.copy_(val)

    x = g["x"]
    our_wrapped.eval()
    with torch.no_grad():
        ol = our_wrapped(input_ids=x, labels=x).loss
    assert torch.allclose(g["loss"], ol, atol=1e-6), (g["loss"], ol)

    # merge semantics identical: same post-merge frozen weights
    our_wrapped.merge_and_reinit()
    ref_w = _group(g, "merged")
    our_w = {n: p for n, p in our_wrapped.named_parameters() if "lora_" not in n}
    assert ref_w
    for n in ref_w:
        assert torch.allclose(ref_w[n], our_w[n], atol=1e-6), n


def test_scheduler_matches_reference():
    from relora_amd import training_utils as our_tu

    with open(os.path.join(GOLDEN, "scheduler.json")) as f:
        cases = json.load(f)
    assert len(cases) == 2
    for case in cases:
        kwargs = case["kwargs"]
        p2 = torch.nn.Parameter(torch.zeros(1))
        o2 = torch.optim.SGD([p2], lr=1.0)
        s2 = our_tu.get_scheculer(optimizer=o2, scheduler_type="cosine_restarts",
                                  **kwargs)
        assert len(case["lrs"]) == kwargs["num_training_steps"]
        for step, ref_lr in enumerate(case["lrs"]):
            assert abs(ref_lr - o2.param_groups[0]["lr"]) < 1e-12, step
            o2.step(); s2.step()


def test_pythia_forward_matches_reference():
    """GPTNeoX: same config + weights -> same loss/grads as the reference."""
    from relora_amd.models.pythia import GPTNeoXConfig, GPTNeoXForCausalLM

    g = _load("pythia_fwd_bwd.npz")
    kw = dict(vocab_size=128, hidden_size=64, num_hidden_layers=2,
              num_attention_heads=4, intermediate_size=256,
              max_position_embeddings=64, rotary_pct=0.25,
              use_parallel_residual=True, tie_word_embeddings=False,
              layer_norm_eps=1e-5)
    ours = GPTNeoXForCausalLM(GPTNeoXConfig(**kw))
    # the reference's state dict without its rotary inv_freq / causal-mask
    # buffers
    missing, unexpected = ours.load_state_dict(_group(g, "w"), strict=False)
    assert not unexpected, unexpected
    assert all("cos_cached" in m or "sin_cached" in m for m in missing), missing

    x = g["x"]
    # NOTE: the reference's eval-mode B>1 path without an attention_mask is
    # NON-CAUSAL (it calls SDPA with attn_mask=None, is_causal=False in that
    # branch) — a reference bug we measured: its own B=2 logits diverge from
    # its B=1 logits by ~0.3.  Ours is causal always (asserted below).  The
    # recorded reference run was given an explicit all-ones mask so that it
    # routed through its correct causal+pad-mask branch.
    am = torch.ones_like(x)
    ours.eval()
    with torch.no_grad():
        rl_ = g["logits"]
        ol_ = ours(input_ids=x, attention_mask=am).logits
        assert torch.allclose(rl_, ol_, atol=2e-5), (rl_ - ol_).abs().max()
        # ours is batch-self-consistent even without a mask (the reference
        # is not, per the bug above)
        ob = ours(input_ids=x).logits
        o0 = ours(input_ids=x[0:1]).logits
        assert torch.allclose(ob[0:1], o0, atol=1e-6)

    our_out = ours(input_ids=x, attention_mask=am, labels=x)
    assert torch.allclose(g["loss_eval"], our_out.loss, atol=2e-5), \
        (g["loss_eval"], our_out.loss)

    # training mode: the reference uses is_causal=True here, so no mask needed
    ours.train()
    ol = ours(input_ids=x, labels=x).loss
    assert torch.allclose(g["loss_train"], ol, atol=2e-5), (g["loss_train"], ol)
    ol.backward()
    ref_grads = _group(g, "g")
    ref_nograd = set(g["nograd"].tolist())
    for n, po in ours.named_parameters():
        assert n in ref_grads or n in ref_nograd, n
        if n in ref_nograd or po.grad is None:
            assert n in ref_nograd and po.grad is None, n
            continue
        assert torch.allclose(ref_grads[n], po.grad, atol=2e-5), n


def test_optimizer_reset_matches_reference():
    from relora_amd import training_utils as our_tu

    g = _load("optimizer_reset.npz")

    # magnitude pruning: identical zeroing pattern
    t2 = g["t"].clone()
    our_tu.magnitude_pruning_(t2, 0.7)
    assert torch.equal(g["t_pruned"], t2)

    # full optimizer_reset with magnitude pruning on the Adam states the
    # reference's optimizer held before its reset
    ps2 = [torch.nn.Parameter(g[f"p/{i}"].clone()) for i in range(3)]
    o2 = torch.optim.Adam(ps2, lr=1e-3)
    for p in ps2:
        p.grad = torch.zeros_like(p)
    o2.step()
    for i, p in enumerate(ps2):
        for k in ("exp_avg", "exp_avg_sq"):
            o2.state[p][k].copy_(g[f"before/{k}/{i}"])
    our_tu.optimizer_reset(o2, reset_params=ps2[:2], optimizer_state_keys=["exp_avg", "exp_avg_sq"],
                           reset_optimizer_on_relora=False, optimizer_random_pruning=0.0,
                           optimizer_magnitude_pruning=0.9)
    for i, p2 in enumerate(ps2):
        s2 = o2.state[p2]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(g[f"after/{k}/{i}"], s2[k])
    # the third parameter was not in reset_params: untouched on both sides
    assert torch.equal(g["after/exp_avg/2"], g["before/exp_avg/2"])


def test_tokenize_and_chunk_matches_reference():
    """HF data path: identical tokenizer + corpus -> identical chunked token
    streams."""
    import datasets as hfds
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    from relora_amd.data.dataloader import tokenize_and_chunk as our_tac

    with open(os.path.join(GOLDEN, "tokenize_and_chunk.json")) as f:
        g = json.load(f)

    words = [f"w{i}" for i in range(40)]
    vocab = {"[PAD]": 0, "[UNK]": 1, "</s>": 2}
    for w in words:
        vocab[w] = len(vocab)
    tok = Tokenizer(models.WordLevel(vocab=vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="[PAD]",
                                   unk_token="[UNK]", eos_token="</s>")

    texts = g["texts"]
    assert len(texts) == 60
    ds_our = hfds.DatasetDict({"train": hfds.Dataset.from_dict({"text": list(texts)})})
    our_out = our_tac(fast, ds_our, "text", 16, num_cpu=1)["train"]

    ref_ids = g["input_ids"]
    assert len(ref_ids) == len(our_out)
    assert set(g["column_names"]) == set(our_out.column_names)
    for i in range(len(ref_ids)):
        assert ref_ids[i] == our_out[i]["input_ids"], i


def _read_json(path, drop=("transformers_version",)):
    with open(path) as f:
        return {k: v for k, v in json.load(f).items() if k not in drop}


def test_checkpoint_cross_compatibility(tmp_path):
    """A user switching frameworks can load checkpoints across: a checkpoint
    written by the REFERENCE's ReLoRaModel.save_pretrained loads through OUR
    ReLoRaModel.from_pretrained with identical forward, and vice versa."""
    from relora_amd.relora import ReLoRaModel as OurReLoRa
    from relora_amd.utils.checkpoint import load_state_dict_compat

    g = _load("checkpoint_losses.npz")
    x = g["x"]

    # reference -> ours: the directory is what the reference's save_pretrained
    # wrote (HF layout, model.safetensors), the loss what it computed from
    # the model it saved
    ours_loaded = OurReLoRa.from_pretrained(
        os.path.join(GOLDEN, "ckpt_written_by_reference"))
    ours_loaded.eval()
    with torch.no_grad():
        ol = ours_loaded(input_ids=x, labels=x).loss
    assert torch.allclose(g["loss_ref"], ol, atol=1e-6), (g["loss_ref"], ol)

    # ours -> reference: ckpt_read_by_reference is a checkpoint our
    # save_pretrained wrote and the reference's from_pretrained loaded;
    # loss_ref_loaded is the loss the reference computed from it.  What we
    # save today must be that same checkpoint (files, configs, tensor names,
    # shapes, dtypes and values), and our loss on it must match.
    recorded = os.path.join(GOLDEN, "ckpt_read_by_reference")
    recorded_sd = load_state_dict_compat(recorded)
    torch.manual_seed(12)
    our_wrapped = OurReLoRa(_our_llama(), **RELORA_KW)
    our_wrapped.wrapped_model.load_state_dict(recorded_sd, strict=True)
    our_dir = tmp_path / "our_ckpt"
    our_wrapped.save_pretrained(str(our_dir))

    assert sorted(os.listdir(our_dir)) == sorted(os.listdir(recorded))
    for name in ("config.json", "relora_config.json"):
        assert _read_json(our_dir / name) == _read_json(os.path.join(recorded, name)), name
    saved_sd = load_state_dict_compat(str(our_dir))
    assert list(saved_sd) == list(recorded_sd)
    for n, v in recorded_sd.items():
        assert saved_sd[n].dtype == v.dtype and torch.equal(saved_sd[n], v), n

    our_wrapped.eval()
    with torch.no_grad():
        ol2 = our_wrapped(input_ids=x, labels=x).loss
    assert torch.allclose(g["loss_ref_loaded"], ol2, atol=1e-6), \
        (g["loss_ref_loaded"], ol2)


def test_megatron_index_builders_match_reference():
    """GPT2Dataset index maps: our builders produce the exact arrays the
    reference's python fallback produces, and the same shuffle/doc orderings
    under the same seed."""
    from relora_amd.data import gpt2_dataset as our_ds

    with np.load(os.path.join(GOLDEN, "megatron_index.npz")) as z:
        g = {k: z[k] for k in z.files}

    # the same trial parameters the recording drew
    rng = np.random.RandomState(0)
    for trial in range(5):
        n_docs = int(rng.randint(2, 50))
        sizes = rng.randint(1, 60, size=n_docs).astype(np.int32)
        seq_length = int(rng.randint(2, 33))
        num_epochs = int(rng.randint(1, 4))
        seed = int(rng.randint(0, 10000))
        np.testing.assert_array_equal(g[f"{trial}/sizes"], sizes)
        assert g[f"{trial}/params"].tolist() == [seq_length, num_epochs, seed]

        np_rng_our = np.random.RandomState(seed)
        documents = np.arange(n_docs, dtype=np.int32)
        doc_idx_ref = g[f"{trial}/doc_idx"]
        doc_idx_our = our_ds._build_doc_idx(documents, num_epochs, np_rng_our)
        assert doc_idx_ref.dtype == doc_idx_our.dtype
        np.testing.assert_array_equal(doc_idx_ref, doc_idx_our)

        tokens_per_epoch = int(sizes.sum())
        ref_sample = g[f"{trial}/sample_idx"]
        our_sample = our_ds.build_sample_idx_py(sizes, doc_idx_our, seq_length,
                                                num_epochs, tokens_per_epoch)
        np.testing.assert_array_equal(ref_sample, our_sample)

        num_samples = ref_sample.shape[0] - 1
        ref_shuffle = g[f"{trial}/shuffle_idx"]
        our_shuffle = our_ds._build_shuffle_idx(num_samples,
                                                np.random.RandomState(seed + 1))
        np.testing.assert_array_equal(ref_shuffle, our_shuffle)
