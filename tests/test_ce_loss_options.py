"""z-loss and label smoothing of the fused cross-entropy, CPU side: the torch
path of the op, the two model families, argument validation and the
trainer's logging.

Objective per valid row (logits x, target t, lse = log sum exp x):
    lse - (1-eps)*x_t - (eps/V)*sum_j x_j + z*lse^2
which for z = 0 is F.cross_entropy(label_smoothing=eps)."""

import json

import pytest
import torch
import torch.nn.functional as F

from relora_amd import ops

OPTIONS = [(1e-2, 0.0), (0.0, 0.25), (1e-2, 0.25)]


def _reference(logits, labels, z, eps):
    """(loss, ce, zl) from materialised logits with plain torch."""
    lse = torch.logsumexp(logits, -1)
    valid = labels != -100
    zl = z * (lse[valid] ** 2).mean()
    loss = F.cross_entropy(logits, labels, label_smoothing=eps, ignore_index=-100) + zl
    return loss, F.cross_entropy(logits, labels, ignore_index=-100), zl


def _inputs(M=64, H=32, V=101):
    torch.manual_seed(0)
    hidden = torch.randn(M, H, requires_grad=True)
    weight = torch.randn(V, H, requires_grad=True)
    labels = torch.randint(0, V, (M,))
    labels[5] = -100
    labels[17] = -100
    return hidden, weight, labels


# ---------------------------------------------------------------------------
# op, torch path
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("chunk", [7, 10_000])
@pytest.mark.parametrize("z,eps", OPTIONS)
def test_torch_path_matches_reference(monkeypatch, chunk, z, eps):
    import relora_amd.ops.functional as fops

    monkeypatch.setattr(fops, "_CE_CHUNK", chunk)
    hidden, weight, labels = _inputs()
    loss = ops.fused_cross_entropy(hidden, weight, labels, z_loss=z, label_smoothing=eps)
    loss.backward()

    h2 = hidden.detach().clone().requires_grad_(True)
    w2 = weight.detach().clone().requires_grad_(True)
    ref, _, _ = _reference(h2 @ w2.t(), labels, z, eps)
    ref.backward()

    assert torch.allclose(loss, ref, atol=1e-5), (loss, ref)
    assert torch.allclose(hidden.grad, h2.grad, atol=1e-5)
    assert torch.allclose(weight.grad, w2.grad, atol=1e-4)
    # ignored rows get an all-zero gradient row
    assert torch.equal(hidden.grad[5], torch.zeros_like(hidden.grad[5]))
    assert torch.equal(hidden.grad[17], torch.zeros_like(hidden.grad[17]))


@pytest.mark.parametrize("chunk", [7, 10_000])
def test_return_parts(monkeypatch, chunk):
    import relora_amd.ops.functional as fops

    monkeypatch.setattr(fops, "_CE_CHUNK", chunk)
    hidden, weight, labels = _inputs()
    z, eps = 1e-2, 0.1
    loss, ce, zl = ops.fused_cross_entropy(hidden, weight, labels, z_loss=z,
                                           label_smoothing=eps, return_parts=True)
    ref, ref_ce, ref_zl = _reference(hidden.detach() @ weight.detach().t(), labels, z, eps)
    assert torch.allclose(loss, ref, atol=1e-5)
    assert torch.allclose(ce, ref_ce, atol=1e-5), (ce, ref_ce)
    assert torch.allclose(zl, ref_zl, atol=1e-5), (zl, ref_zl)
    assert loss.requires_grad
    assert not ce.requires_grad and not zl.requires_grad
    loss.backward()  # the parts do not take part in backward
    assert hidden.grad is not None


def test_return_parts_options_off():
    hidden, weight, labels = _inputs()
    plain = ops.fused_cross_entropy(hidden, weight, labels)
    loss, ce, zl = ops.fused_cross_entropy(hidden, weight, labels, return_parts=True)
    assert torch.equal(loss, plain) and torch.equal(ce, plain)
    assert zl.item() == 0.0
    assert not ce.requires_grad and not zl.requires_grad


def test_explicit_zeros_are_the_plain_path():
    hidden, weight, labels = _inputs()
    a = ops.fused_cross_entropy(hidden, weight, labels)
    a.backward()
    ga, gw = hidden.grad.clone(), weight.grad.clone()
    hidden.grad = weight.grad = None
    b = ops.fused_cross_entropy(hidden, weight, labels, z_loss=0.0, label_smoothing=0.0)
    b.backward()
    assert torch.equal(a, b)
    assert torch.equal(ga, hidden.grad) and torch.equal(gw, weight.grad)


@pytest.mark.parametrize("kw", [{"z_loss": -1.0}, {"label_smoothing": 1.0},
                                {"label_smoothing": -0.1}])
def test_op_rejects_bad_options(kw):
    hidden, weight, labels = _inputs()
    with pytest.raises(ValueError):
        ops.fused_cross_entropy(hidden, weight, labels, **kw)


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------


def _model(family, request):
    if family == "llama":
        from relora_amd.models.llama import LlamaForCausalLM
        cfg = request.getfixturevalue("tiny_llama_config")
        return LlamaForCausalLM(cfg), cfg
    from relora_amd.models.pythia import GPTNeoXForCausalLM
    cfg = request.getfixturevalue("tiny_pythia_config")
    return GPTNeoXForCausalLM(cfg), cfg


@pytest.mark.parametrize("family", ["llama", "pythia"])
def test_model_fused_equals_unfused_with_options(family, request):
    torch.manual_seed(0)
    model, cfg = _model(family, request)
    z, eps = 1e-2, 0.1
    model.set_loss_options(z_loss=z, label_smoothing=eps)
    model.train()
    x = torch.randint(0, cfg.vocab_size, (2, 24))
    fused = model(input_ids=x, labels=x)
    model.fused_ce = False
    unfused = model(input_ids=x, labels=x)
    assert torch.allclose(fused.loss, unfused.loss, atol=1e-5), (fused.loss, unfused.loss)
    assert torch.allclose(fused.ce_loss, unfused.ce_loss, atol=1e-5)
    assert torch.allclose(fused.z_loss, unfused.z_loss, atol=1e-5)
    assert not fused.ce_loss.requires_grad and not fused.z_loss.requires_grad

    # and both are the documented objective of the model's own logits
    logits = unfused.logits[:, :-1].reshape(-1, cfg.vocab_size).detach()
    ref, ref_ce, ref_zl = _reference(logits, x[:, 1:].reshape(-1), z, eps)
    assert torch.allclose(fused.loss, ref, atol=1e-5)
    assert torch.allclose(fused.ce_loss, ref_ce, atol=1e-5)
    assert torch.allclose(fused.z_loss, ref_zl, atol=1e-5)
    # the options move the loss: z * lse^2 alone is > 0.01 * ln(V)^2 / 2
    assert (fused.loss - fused.ce_loss).item() > 0.05


@pytest.mark.parametrize("family", ["llama", "pythia"])
@pytest.mark.parametrize("fused_ce", [True, False])
def test_model_eval_ignores_options(family, fused_ce, request):
    torch.manual_seed(0)
    model, cfg = _model(family, request)
    model.fused_ce = fused_ce
    x = torch.randint(0, cfg.vocab_size, (2, 24))
    model.eval()
    with torch.no_grad():
        plain = model(input_ids=x, labels=x)
        model.set_loss_options(z_loss=1e-2, label_smoothing=0.1)
        with_options = model(input_ids=x, labels=x)
    assert torch.equal(plain.loss, with_options.loss)
    assert with_options.ce_loss is None and with_options.z_loss is None
    # the options come back with training mode
    model.train()
    out = model(input_ids=x, labels=x)
    assert out.loss.item() > plain.loss.item() + 0.05
    assert out.ce_loss is not None and out.z_loss is not None
    # and default options give no parts
    model.set_loss_options()
    out = model(input_ids=x, labels=x)
    assert out.ce_loss is None and out.z_loss is None
    assert torch.allclose(out.loss, plain.loss, atol=1e-6)


@pytest.mark.parametrize("family", ["llama", "pythia"])
def test_model_rejects_bad_options(family, request):
    model, _ = _model(family, request)
    assert model.z_loss == 0.0 and model.label_smoothing == 0.0
    for kw in ({"z_loss": -1.0}, {"label_smoothing": 1.0}, {"label_smoothing": -0.1}):
        with pytest.raises(ValueError):
            model.set_loss_options(**kw)
    assert model.z_loss == 0.0 and model.label_smoothing == 0.0


@pytest.mark.parametrize("family", ["llama", "pythia"])
def test_options_survive_relora_wrapping(family, request):
    from relora_amd.relora import ReLoRaModel

    torch.manual_seed(0)
    model, cfg = _model(family, request)
    x = torch.randint(0, cfg.vocab_size, (2, 24))
    model.eval()
    with torch.no_grad():
        plain = model(input_ids=x, labels=x).loss
    model.set_loss_options(z_loss=1e-2, label_smoothing=0.1)
    wrapped = ReLoRaModel(model, r=4, lora_alpha=32, lora_dropout=0.0,
                          target_modules=["attn", "attention", "mlp"],
                          keep_original_weights=True)
    wrapped.train()
    out = wrapped(input_ids=x, labels=x)
    # lora_B starts at zero, so the wrapped model computes the same logits
    assert out.ce_loss is not None and torch.allclose(out.ce_loss, plain, atol=1e-5)
    assert out.loss.item() > plain.item() + 0.05
    wrapped.eval()
    with torch.no_grad():
        assert torch.allclose(wrapped(input_ids=x, labels=x).loss, plain, atol=1e-6)
    # the wrapper's own setter reaches the wrapped model
    wrapped.set_loss_options(z_loss=0.0, label_smoothing=0.0)
    assert model.z_loss == 0.0 and model.label_smoothing == 0.0
    wrapped.set_loss_options(z_loss=2e-2)
    assert model.z_loss == 2e-2


@pytest.mark.parametrize("family", ["llama", "pythia"])
def test_options_stay_out_of_config_json(family, request, tmp_path):
    """The checkpoint layout the project writes (ReLoRaModel.save_pretrained:
    config.json, pytorch_model.bin, relora_config.json) is the same with and
    without options, and a loaded model starts with the defaults."""
    from relora_amd.relora import ReLoRaModel

    model, cfg = _model(family, request)
    wrapped = ReLoRaModel(model, r=4, lora_alpha=32, lora_dropout=0.0,
                          target_modules=["attn", "attention", "mlp"],
                          keep_original_weights=True)
    wrapped.save_pretrained(str(tmp_path / "plain"))
    keys_plain = set(wrapped.state_dict())
    wrapped.set_loss_options(z_loss=1e-2, label_smoothing=0.1)
    wrapped.save_pretrained(str(tmp_path / "opts"))
    assert set(wrapped.state_dict()) == keys_plain
    for name in ("config.json", "relora_config.json"):
        a = json.load(open(tmp_path / "plain" / name))
        b = json.load(open(tmp_path / "opts" / name))
        assert a == b, name
        assert not any("z_loss" in k or "smoothing" in k for k in b), name
    loaded = ReLoRaModel.from_pretrained(str(tmp_path / "opts"))
    assert loaded.wrapped_model.z_loss == 0.0
    assert loaded.wrapped_model.label_smoothing == 0.0


# ---------------------------------------------------------------------------
# args
# ---------------------------------------------------------------------------

_ARGS = ["--synthetic_data", "true", "--batch_size", "4"]


def test_args_defaults_and_values():
    from relora_amd.trainer import parse_args

    args = parse_args(_ARGS)
    assert args.z_loss == 0.0 and args.label_smoothing == 0.0
    args = parse_args(_ARGS + ["--z_loss", "1e-2", "--label_smoothing", "0.1"])
    assert args.z_loss == 1e-2 and args.label_smoothing == 0.1


@pytest.mark.parametrize("extra", [["--z_loss", "-1"], ["--label_smoothing", "1.0"],
                                   ["--label_smoothing", "-0.1"]])
def test_args_reject_bad_options(extra):
    from relora_amd.trainer import parse_args

    with pytest.raises(ValueError):
        parse_args(_ARGS + extra)


def test_args_yaml_override(tmp_path):
    from relora_amd.trainer import parse_args

    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("synthetic_data: true\nbatch_size: 4\nz_loss: 1e-2\nlabel_smoothing: 0.1\n")
    args = parse_args(["--training_config", str(cfg)])
    assert args.z_loss == 1e-2 and args.label_smoothing == 0.1
    cfg.write_text("synthetic_data: true\nbatch_size: 4\nlabel_smoothing: 1.5\n")
    with pytest.raises(ValueError):
        parse_args(["--training_config", str(cfg)])


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------


@pytest.fixture
def _single_proc_env(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    yield
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def _run(tmp_path, extra):
    """3 update steps of 2 micro-batches each on llama_9m, ReLoRA-wrapped,
    with a final evaluation; returns the offline wandb records."""
    from relora_amd.trainer import main, parse_args

    main(parse_args([
        "--model_config", "configs/llama_9m.json",
        "--synthetic_data", "true",
        "--use_peft", "true", "--relora", "3", "--cycle_length", "3",
        "--restart_warmup_steps", "1", "--scheduler", "cosine_restarts",
        "--warmup_steps", "2", "--num_training_steps", "3",
        "--batch_size", "2", "--total_batch_size", "4",
        "--max_length", "32", "--lr", "1e-3", "--dtype", "float32",
        "--eval_every", "100", "--save_every", "100", "--workers", "0",
        "--save_dir", str(tmp_path / "run"),
    ] + extra))
    return [json.loads(l) for l in open(tmp_path / "run" / "wandb_offline.jsonl")]


def test_trainer_logs_loss_parts(tmp_path, _single_proc_env, monkeypatch):
    from relora_amd import trainer

    # keep the model the trainer evaluates last, to evaluate it again below
    seen = {}
    real_eval = trainer.evaluate_model

    def spy(model, loader, device, **kw):
        seen["model"], seen["loader"], seen["device"], seen["kw"] = model, loader, device, kw
        seen["result"] = real_eval(model, loader, device, **kw)
        return seen["result"]

    monkeypatch.setattr(trainer, "evaluate_model", spy)
    logged = _run(tmp_path, ["--z_loss", "1e-2", "--label_smoothing", "0.1"])

    updates = [r for r in logged if "loss" in r]
    assert [r["update_step"] for r in updates] == [1, 2, 3]
    for r in updates:
        assert "ce_loss" in r and "z_loss" in r
        assert r["z_loss"] > 0
        assert r["loss"] >= r["ce_loss"]
        # z * lse^2 with lse >= ln(V)/2 or so: the terms are not noise
        assert r["loss"] - r["ce_loss"] > 0.05

    # the trained model still carries the options, and eval does not see them
    model = seen["model"]
    base = model.module.wrapped_model
    assert base.z_loss == 1e-2 and base.label_smoothing == 0.1
    final = [r for r in logged if "final_eval_loss" in r][-1]["final_eval_loss"]
    base.set_loss_options()
    cleared, _ = real_eval(model, seen["loader"], seen["device"], **seen["kw"])
    assert float(cleared) == float(seen["result"][0]) == final


def test_trainer_without_flags_logs_todays_keys(tmp_path, _single_proc_env):
    logged = _run(tmp_path, [])
    updates = [r for r in logged if "loss" in r]
    assert len(updates) == 3
    for r in updates:
        assert list(r) == ["loss", "lr", "update_step", "tokens_seen", "throughput_tokens",
                           "throughput_examples", "throughput_batches", "n_lora_restarts",
                           "n_optimizer_resets", "_step"]
    assert not any("ce_loss" in r or "z_loss" in r for r in logged)
