"""Per-head QK RMSNorm (config.qk_norm) above the kernels, on the CPU: config
round trip, Qwen3 checkpoint interchange in both directions, the torch path's
gradients, save/load, ReLoRA, `.generate()`, the trainer flag and the memory
estimate."""

import json
import os

import pytest
import torch

import qk_norm_common as qc
from relora_amd import ops
from relora_amd.models.config import LlamaConfig, load_model_config
from relora_amd.models.llama import LlamaForCausalLM, LlamaForSequenceClassification
from relora_amd.utils.checkpoint import save_pretrained_compat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_config(**kw):
    d = dict(vocab_size=128, hidden_size=64, intermediate_size=96,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             max_position_embeddings=64, bos_token_id=0, eos_token_id=1,
             rms_norm_eps=1e-6, qk_norm=True)
    d.update(kw)
    return LlamaConfig(**d)


def _randomize_norms(model, seed=7):
    """q_norm / k_norm start at ones; give them values a test can see"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "q_norm" in n or "k_norm" in n:
                p.copy_(1 + 0.5 * torch.randn(p.shape, generator=g))


# -- 1. config ------------------------------------------------------------------

def test_config_round_trip(tmp_path):
    off = tiny_config(qk_norm=False)
    assert off.qk_norm is False and "qk_norm" not in off.to_dict()
    assert "qk_norm" not in json.loads(off.to_json_string(use_diff=False))
    assert LlamaConfig().qk_norm is False
    off.save_pretrained(tmp_path / "off")
    with open(tmp_path / "off" / "config.json") as f:
        assert "qk_norm" not in json.load(f)
    assert load_model_config(str(tmp_path / "off")).qk_norm is False

    on = tiny_config()
    assert on.to_dict()["qk_norm"] is True
    on.save_pretrained(tmp_path / "on")
    with open(tmp_path / "on" / "config.json") as f:
        assert json.load(f)["qk_norm"] is True
    assert load_model_config(str(tmp_path / "on")).qk_norm is True
    assert LlamaConfig.from_pretrained(tmp_path / "on").qk_norm is True

    # a model without the option has no norm modules and today's keys
    keys = set(LlamaForCausalLM(off).state_dict())
    assert not any("q_norm" in k or "k_norm" in k for k in keys)
    keys_on = set(LlamaForCausalLM(on).state_dict())
    extra = keys_on - keys
    assert extra == {f"model.layers.{i}.self_attn.{n}_norm.weight"
                     for i in range(2) for n in "qk"}
    attn = LlamaForCausalLM(on).model.layers[0].self_attn
    assert attn.q_norm.weight.shape == (16,) and attn.k_norm.weight.shape == (16,)
    assert attn.q_norm.variance_epsilon == on.rms_norm_eps


def test_existing_config_files_are_written_as_before(tmp_path):
    """every shipped LLaMA config loads with the option off and is written
    back without the field"""
    import glob

    n = 0
    for f in sorted(glob.glob(os.path.join(REPO, "configs", "*.json"))):
        with open(f) as fh:
            if json.load(fh).get("model_type", "llama") != "llama":
                continue
        cfg = load_model_config(f)
        assert cfg.qk_norm is False, f
        assert "qk_norm" not in cfg.to_dict(), f
        n += 1
    assert n >= 15


# -- 2. Qwen3 parity ------------------------------------------------------------

def _qwen3_tiny():
    import transformers

    cfg = transformers.Qwen3Config(
        vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=2, head_dim=16,
        max_position_embeddings=64, rms_norm_eps=1e-6, rope_theta=10000.0,
        tie_word_embeddings=False, attention_bias=False, bos_token_id=0, eos_token_id=1,
        pad_token_id=None, use_sliding_window=False)
    cfg._attn_implementation = "sdpa"   # the arithmetic of this project's CPU path
    torch.manual_seed(0)
    return transformers.Qwen3ForCausalLM(cfg).float().eval()


def _same_logits(m1, m2, x, what):
    """the criterion of test_gqa_models.py::test_hf_checkpoint_interchange_exact"""
    with torch.no_grad():
        a, b = m1(input_ids=x).logits, m2(input_ids=x).logits
    print(what, "max |dlogits|", (a - b).abs().max().item())
    assert torch.equal(a, b), (what, (a - b).abs().max())


def test_qwen3_parity_both_directions():
    x = torch.randint(0, 128, (2, 12), generator=torch.Generator().manual_seed(1))
    hf = _qwen3_tiny()
    _randomize_norms(hf)
    ours = LlamaForCausalLM(tiny_config()).eval()
    ours.load_state_dict(hf.state_dict(), strict=True)
    _same_logits(hf, ours, x, "qwen3->ours")
    # the norm is in force: without its weights the logits move
    plain = LlamaForCausalLM(tiny_config(qk_norm=False)).eval()
    plain.load_state_dict(hf.state_dict(), strict=False)
    with torch.no_grad():
        assert not torch.equal(plain(input_ids=x).logits, ours(input_ids=x).logits)

    torch.manual_seed(5)
    mine = LlamaForCausalLM(tiny_config()).eval()
    _randomize_norms(mine, seed=9)
    hf2 = _qwen3_tiny()
    hf2.load_state_dict(mine.state_dict(), strict=True)
    _same_logits(mine, hf2, x, "ours->qwen3")


# -- 3. torch path --------------------------------------------------------------

def test_torch_path_gradcheck():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(2, 1, 5, 8, generator=g, dtype=torch.float64, requires_grad=True)
    wq = (1 + 0.5 * torch.randn(8, generator=g, dtype=torch.float64)).requires_grad_()
    wk = (1 + 0.5 * torch.randn(8, generator=g, dtype=torch.float64)).requires_grad_()
    cos, sin = (t.double() for t in ops.build_rope_cache(8, 7))
    # rmsnorm_torch takes the variance of x.to(float32) whatever the input's
    # dtype (the reference model's numerics), so a function value carries an
    # error of about 2^-23 |y|, 5e-7 at |y| <= 4.  A central difference with
    # step h divides that by 2h and adds a truncation error h^2 |f3| / 6, the
    # third derivative f3 of order 10 for rows of 8 unit-scale entries: at
    # h = 1e-2 that is 2.5e-5 of noise and 2e-4 of truncation.  Hence step
    # 1e-2 and atol 5e-4; a wrong term in the gradient is an error of order
    # 0.01 to 1.
    tol = dict(eps=1e-2, atol=5e-4, rtol=1e-3)
    assert torch.autograd.gradcheck(
        lambda *a: ops.qk_norm_rope_torch(*a, cos, sin, 1e-3), (q, k, wq, wk), **tol)
    # position_ids: the kv-cache path
    pos = torch.tensor([[2, 3, 4, 5, 6]])
    assert torch.autograd.gradcheck(
        lambda *a: ops.qk_norm_rope_torch(*a, cos, sin, 1e-3, pos), (q, k, wq, wk), **tol)


def test_torch_path_matches_reference_and_dispatch():
    """the CPU call of ops.qk_norm_rope is the torch composition, and that is
    the float64 reference's chain"""
    x, w, dy = qc.make_case(2, 3, 9, 16, seed=3)
    xk, wk, dyk = qc.make_case(2, 1, 9, 16, seed=4)
    cos, sin = ops.build_rope_cache(16, 12)
    q, k = x.double().requires_grad_(), xk.double().requires_grad_()
    wq_, wk_ = w.double().requires_grad_(), wk.double().requires_grad_()
    qo, ko = ops.qk_norm_rope(q, k, wq_, wk_, cos.double(), sin.double(), 1e-5)
    torch.autograd.backward((qo, ko), (dy.double(), dyk.double()))
    for got, gx, gw, (xx, ww, dd) in ((qo, q.grad, wq_.grad, (x, w, dy)),
                                      (ko, k.grad, wk_.grad, (xk, wk, dyk))):
        ref = qc.reference(xx, ww, dd, cos, sin, 1e-5)
        # the fp32 variance of rmsnorm_torch: a few 2^-24 relative
        assert (got - ref["out"]).abs().max() <= 1e-6 * ref["out"].abs().max()
        assert (gx - ref["dx"]).abs().max() <= 1e-6 * ref["dx"].abs().max()
        assert (gw - ref["dw"]).abs().max() <= 1e-6 * ref["dw"].abs().max()
    # all-zero row: output 0, finite gradients
    assert torch.equal(qo[1, 2, 4], torch.zeros(16, dtype=torch.float64))
    assert torch.isfinite(q.grad).all()


# -- 4. model -------------------------------------------------------------------

def test_save_and_from_pretrained_round_trip(tmp_path):
    torch.manual_seed(1)
    model = LlamaForCausalLM(tiny_config()).eval()
    _randomize_norms(model)
    x = torch.randint(0, 128, (2, 10), generator=torch.Generator().manual_seed(2))
    save_pretrained_compat(model, str(tmp_path / "m"))
    with open(tmp_path / "m" / "config.json") as f:
        assert json.load(f)["qk_norm"] is True
    again = LlamaForCausalLM.from_pretrained(tmp_path / "m").eval()
    assert again.config.qk_norm is True
    a = model.model.layers[1].self_attn.k_norm.weight
    b = again.model.layers[1].self_attn.k_norm.weight
    assert torch.equal(a, b) and not torch.equal(a, torch.ones_like(a))
    with torch.no_grad():
        assert torch.equal(model(input_ids=x).logits, again(input_ids=x).logits)


def test_relora_wrap_merge_round_trip(tmp_path):
    from relora_amd.relora import ReLoRaModel

    torch.manual_seed(0)
    base = LlamaForCausalLM(tiny_config())
    _randomize_norms(base)
    model = ReLoRaModel(base, r=8, lora_alpha=32, lora_dropout=0.0,
                        target_modules=["attn", "attention", "mlp"],
                        keep_original_weights=True)
    norms = {n: p for n, p in model.named_parameters() if "q_norm" in n or "k_norm" in n}
    assert len(norms) == 4 and all(p.requires_grad for p in norms.values())
    assert all(type(m).__name__ == "LlamaRMSNorm"
               for n, m in model.named_modules() if n.endswith(("q_norm", "k_norm")))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.normal_(std=0.05)
    x = torch.randint(0, 128, (2, 10), generator=torch.Generator().manual_seed(2))
    # the norm weights get gradients through the wrapped projections
    model.train()
    model(input_ids=x, labels=x).loss.backward()
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in norms.values())
    model.eval()
    kept = {n: p.detach().clone() for n, p in norms.items()}
    with torch.no_grad():
        before = model(input_ids=x).logits
        model.merge_and_reinit()
        merged = model(input_ids=x).logits
    assert (before - merged).abs().max() <= 1e-5
    for n, p in model.named_parameters():
        if n in kept:
            assert torch.equal(p, kept[n]) and p.requires_grad, n
    model.save_pretrained(str(tmp_path))
    again = ReLoRaModel.from_pretrained(str(tmp_path)).eval()
    with torch.no_grad():
        assert torch.equal(merged, again(input_ids=x).logits)
    for n, p in again.named_parameters():
        if n in kept:
            assert torch.equal(p, kept[n]) and p.requires_grad, n


def test_generate_matches_manual_greedy():
    torch.manual_seed(0)
    x = torch.randint(2, 128, (1, 5))
    m = LlamaForCausalLM(tiny_config()).eval()
    _randomize_norms(m)
    out = m.generate(x, max_new_tokens=6, do_sample=False)
    cur = x.clone()
    for _ in range(6):
        with torch.no_grad():
            cur = torch.cat([cur, m(input_ids=cur).logits[:, -1:].argmax(-1)], dim=1)
    assert torch.equal(out, cur)
    with torch.no_grad():
        full = m(input_ids=cur).logits
        pre = m(input_ids=cur[:, :-1], use_cache=True)
        step = m(input_ids=cur[:, -1:], past_key_values=pre.past_key_values,
                 use_cache=True).logits
    assert (step[:, -1] - full[:, -1]).abs().max() <= 1e-5


def test_sequence_classification_and_checkpointing_cpu():
    torch.manual_seed(0)
    x = torch.randint(2, 128, (2, 9))
    cls = LlamaForSequenceClassification(tiny_config(num_labels=3)).train()
    out = cls(input_ids=x, labels=torch.tensor([0, 2]))
    out.loss.backward()
    assert cls.model.layers[0].self_attn.q_norm.weight.grad is not None

    m = LlamaForCausalLM(tiny_config()).train()
    _randomize_norms(m)
    m(input_ids=x, labels=x).loss.backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    m.model.gradient_checkpointing = True
    m(input_ids=x, labels=x).loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, want[n]), n


# -- trainer flag -----------------------------------------------------------------

def _base_args(tmp_path, model_args):
    return model_args + [
        "--synthetic_data", "true", "--batch_size", "2", "--total_batch_size", "2",
        "--max_length", "32", "--dtype", "float32", "--save_dir", str(tmp_path / "run")]


def test_trainer_flag_parses_and_pythia_is_rejected(tmp_path):
    from relora_amd.trainer import parse_args, resolve_qk_norm

    llama = ["--model_config", "configs/llama_9m.json"]
    assert parse_args(_base_args(tmp_path, llama)).qk_norm is None
    assert parse_args(_base_args(tmp_path, llama) + ["--qk_norm", "true"]).qk_norm is True
    assert parse_args(_base_args(tmp_path, llama) + ["--qk_norm", "false"]).qk_norm is False
    pythia = ["--model_config", "configs/pythia_160m.json"]
    parse_args(_base_args(tmp_path, pythia))   # Pythia alone is fine
    for v in ("true", "false"):
        with pytest.raises(ValueError, match="qk_norm"):
            parse_args(_base_args(tmp_path, pythia) + ["--qk_norm", v])

    # the flag sets the field of a freshly built config
    args = parse_args(_base_args(tmp_path, llama) + ["--qk_norm", "true"])
    cfg = load_model_config(os.path.join(REPO, "configs", "llama_9m.json"))
    assert resolve_qk_norm(args, cfg, from_checkpoint=False) is True and cfg.qk_norm is True
    # no flag: the config is left alone
    cfg = load_model_config(os.path.join(REPO, "configs", "llama_9m.json"))
    none = parse_args(_base_args(tmp_path, llama))
    assert resolve_qk_norm(none, cfg, from_checkpoint=False) is False
    assert "qk_norm" not in cfg.to_dict()
    from relora_amd.models.config import GPTNeoXConfig
    with pytest.raises(ValueError, match="LLaMA"):
        resolve_qk_norm(args, GPTNeoXConfig(), from_checkpoint=False)


def test_trainer_flag_against_checkpoint_config(tmp_path):
    from relora_amd.trainer import parse_args, resolve_qk_norm

    for saved in (True, False):
        d = tmp_path / f"ckpt_{saved}"
        save_pretrained_compat(LlamaForCausalLM(tiny_config(qk_norm=saved)), str(d))
        model_args = ["--model_name_or_path", str(d)]
        cfg = load_model_config(str(d))
        # the checkpoint's config decides
        args = parse_args(_base_args(tmp_path, model_args))
        assert resolve_qk_norm(args, cfg, from_checkpoint=True) is saved
        same = parse_args(_base_args(tmp_path, model_args) + ["--qk_norm", str(saved).lower()])
        assert resolve_qk_norm(same, cfg, from_checkpoint=True) is saved
        other = parse_args(_base_args(tmp_path, model_args)
                           + ["--qk_norm", str(not saved).lower()])
        with pytest.raises(ValueError, match="conflicts"):
            resolve_qk_norm(other, cfg, from_checkpoint=True)
        assert cfg.qk_norm is saved


@pytest.fixture
def _single_proc_env(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    yield
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def test_trainer_runs_with_flag_and_rejects_conflict(tmp_path, _single_proc_env):
    """--qk_norm true trains a LLaMA with the norm weights among the trainable
    parameters and saves them; resuming that run's weights into a config
    without the option is rejected"""
    import torch.distributed as dist

    from relora_amd import trainer

    def args(sub, extra):
        return trainer.parse_args([
            "--model_config", "configs/llama_9m.json", "--synthetic_data", "true",
            "--use_peft", "true", "--relora", "3", "--cycle_length", "3",
            "--restart_warmup_steps", "1", "--scheduler", "cosine_restarts",
            "--num_training_steps", "6", "--warmup_steps", "2",
            "--batch_size", "2", "--total_batch_size", "2", "--max_length", "32",
            "--lr", "1e-3", "--dtype", "float32", "--eval_every", "100",
            "--save_every", "100", "--workers", "0", "--lora_r", "8",
            "--save_dir", str(tmp_path / sub)] + extra)

    trainer.main(args("on", ["--qk_norm", "true"]))
    if dist.is_initialized():
        dist.destroy_process_group()
    ckpt = tmp_path / "on" / "model_6"
    with open(ckpt / "config.json") as f:
        assert json.load(f)["qk_norm"] is True
    sd = torch.load(ckpt / "pytorch_model.bin", map_location="cpu", weights_only=True)
    norm_keys = [k for k in sd if "q_norm" in k or "k_norm" in k]
    assert len(norm_keys) == 2 * load_model_config("configs/llama_9m.json").num_hidden_layers
    # trained: no longer the initial ones
    assert any(not torch.equal(sd[k], torch.ones_like(sd[k])) for k in norm_keys)
    with pytest.raises(ValueError, match="conflicts"):
        trainer.main(args("off", ["--qk_norm", "false", "--warmed_up_model", str(ckpt)]))
    if dist.is_initialized():
        dist.destroy_process_group()


# -- memory ---------------------------------------------------------------------

def test_memory_estimate():
    from relora_amd.utils import memory

    for name in ("llama_250m.json", "llama_1b_gqa.json"):
        f = os.path.join(REPO, "configs", name)
        off, on = load_model_config(f), load_model_config(f)
        on.qk_norm = True
        L, H, nh = off.num_hidden_layers, off.hidden_size, off.num_attention_heads
        nkv, hd = off.num_key_value_heads, off.hidden_size // off.num_attention_heads
        # off: the figures of the code before the option (no such attribute)
        bare = load_model_config(f)
        del bare.qk_norm
        for bs in (1, 8):
            assert (memory.estimate_step_bytes(off, bs, 2048, lora_r=128)
                    == memory.estimate_step_bytes(bare, bs, 2048, lora_r=128))
        assert memory.estimate_param_count(off, 128) == memory.estimate_param_count(bare, 128)
        n_off, _ = memory.estimate_param_count(off)
        n_on, _ = memory.estimate_param_count(on)
        assert n_on - n_off == 2 * L * hd
        with torch.device("meta"):
            assert sum(p.numel() for p in LlamaForCausalLM(on).parameters()) == n_on
        T = 8 * 2048
        extra = (memory.estimate_step_bytes(on, 8, 2048, lora_r=128, trainable_ratio=0.0)
                 - memory.estimate_step_bytes(off, 8, 2048, lora_r=128, trainable_ratio=0.0))
        # pre-norm q and k in bf16, two fp32 invrms per layer, and the weights
        want = L * (T * (H + nkv * hd) * 2 + T * (nh + nkv) * 4) + 2 * L * hd * 2
        assert extra == want, (extra, want)
