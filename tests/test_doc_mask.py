"""Intra-document attention masking, CPU side: `ops.doc_starts_from_eos`, the
masked SDPA path (`sdpa_torch(doc_start=...)`, the torch oracle and the path
for everything the HIP doc kernels do not take), `flash_attention` argument
checks, the LLaMA model's `forward(doc_start=...)`, the trainer flag, and the
conditioning of the GPU tests' inputs."""

import pytest
import torch

import attn_variant_worker as aw
import docmask_common as dc
import gqa_common as gc

from relora_amd import ops
from relora_amd.ops import functional as Fn


# ---- doc_starts_from_eos ---------------------------------------------------

EOS = 9


@pytest.mark.parametrize("ids, want", [
    ([1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0]),             # no eos
    ([EOS, 2, 3, 4, 5, 6], [0, 1, 1, 1, 1, 1]),           # eos at position 0
    ([1, 2, 3, 4, 5, EOS], [0, 0, 0, 0, 0, 0]),           # eos at the last position
    ([1, EOS, EOS, EOS, 5, 6], [0, 0, 2, 3, 4, 4]),       # consecutive eos
    ([1, 2, EOS, 4, EOS, 6], [0, 0, 0, 3, 3, 5]),
])
def test_doc_starts_from_eos(ids, want):
    ds = ops.doc_starts_from_eos(torch.tensor([ids]), EOS)
    assert ds.dtype == torch.int32 and ds.shape == (1, len(ids))
    assert ds.tolist() == [want]
    assert dc.is_well_formed(ds)


def test_doc_starts_from_eos_batch_rows_differ():
    ids = torch.tensor([[1, EOS, 3, 4, EOS, 6, 7, 8],
                        [EOS, 2, 3, EOS, EOS, 6, 7, EOS],
                        [1, 2, 3, 4, 5, 6, 7, 8]])
    ds = ops.doc_starts_from_eos(ids, EOS)
    assert ds.dtype == torch.int32 and ds.is_contiguous()
    assert ds.tolist() == [[0, 0, 2, 2, 2, 5, 5, 5],
                           [0, 1, 1, 1, 4, 5, 5, 5],
                           [0, 0, 0, 0, 0, 0, 0, 0]]
    assert dc.is_well_formed(ds)
    g = torch.Generator().manual_seed(0)
    big = torch.randint(0, 12, (4, 257), generator=g)
    assert dc.is_well_formed(ops.doc_starts_from_eos(big, EOS))


# ---- masked SDPA -----------------------------------------------------------

def _dense_per_document(q, k, v, rows):
    """plain causal attention run on every document's slice separately"""
    out = torch.empty_like(q)
    for b, lengths in enumerate(rows):
        pos = 0
        for n in lengths:
            sl = slice(pos, pos + n)
            out[b:b + 1, :, sl] = Fn.sdpa_torch(q[b:b + 1, :, sl], k[b:b + 1, :, sl],
                                                v[b:b + 1, :, sl], causal=True)
            pos += n
    return out


@pytest.mark.parametrize("nkv", [4, 2])
def test_sdpa_doc_start_equals_per_document_loop(nkv):
    rows = ([5, 1, 20, 6], [32])
    ds = dc.doc_start_from_lengths(rows, 32)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, 4, 32, 16, generator=g, dtype=torch.float64)
    k = torch.randn(2, nkv, 32, 16, generator=g, dtype=torch.float64)
    v = torch.randn(2, nkv, 32, 16, generator=g, dtype=torch.float64)
    got = Fn.sdpa_torch(q, k, v, doc_start=ds)
    want = _dense_per_document(q, k, v, rows)
    assert (got - want).abs().max().item() < 1e-12
    # and through the public entry point (CPU -> SDPA)
    assert torch.equal(ops.flash_attention(q, k, v, doc_start=ds), got)
    assert torch.equal(ops.doc_mask(ds, 32), dc.allowed(ds))


def test_zero_doc_start_is_plain_causal():
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(2, 4, 40, 16, generator=g) for _ in range(3))
    ds = torch.zeros(2, 40, dtype=torch.int32)
    assert torch.equal(ops.flash_attention(q, k, v, doc_start=ds),
                       ops.flash_attention(q, k, v))


def test_flash_attention_argument_errors():
    q = torch.randn(2, 4, 8, 16)
    ds = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="causal"):
        ops.flash_attention(q, q, q, causal=False, doc_start=ds)
    k = torch.randn(2, 4, 12, 16)
    with pytest.raises(ValueError, match="equal q and kv lengths"):
        ops.flash_attention(q, k, k, doc_start=ds)
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        ops.flash_attention(q, q, q, doc_start=ds[:1])
    with pytest.raises(ValueError, match="int32"):
        ops.flash_attention(q, q, q, doc_start=ds.long())


# ---- model -----------------------------------------------------------------

def _tiny(cfg, seed=0):
    from relora_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(seed)
    return LlamaForCausalLM(cfg).float().eval()


# fp32 difference between document B's logits inside the packed row and
# alone, measured on the CPU (max abs; logits are O(0.1)): RoPE rotates q
# and k of the packed B by 40 more positions each, so the scores agree only
# up to fp32 rounding of the rotation.
PACKED_VS_ALONE_MEASURED = 2.1e-7
PACKED_VS_ALONE_BOUND = 10 * PACKED_VS_ALONE_MEASURED


def test_packed_document_equals_document_alone(tiny_llama_config):
    """Logits of document B in the packed row [A; B] with doc_start equal the
    logits of [B] alone: RoPE positions are not reset, but the scores depend
    only on i - j.  Measured fp32 difference 2.1e-7 (max abs), bound 10x that
    = 2.1e-6; without doc_start the same logits differ by 0.53 (measured),
    asserted to be more than 1000x the bound."""
    model = _tiny(tiny_llama_config)
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, 256, (1, 40), generator=g)
    b = torch.randint(0, 256, (1, 56), generator=g)
    packed = torch.cat([a, b], dim=1)
    ds = dc.doc_start_from_lengths(([40, 56],), 96)
    with torch.no_grad():
        alone = model(input_ids=b).logits
        masked = model(input_ids=packed, doc_start=ds).logits[:, 40:]
        leaky = model(input_ids=packed).logits[:, 40:]
        also_a = model(input_ids=packed, doc_start=ds).logits[:, :40]
        a_alone = model(input_ids=a).logits
    diff = (masked - alone).abs().max().item()
    leak = (leaky - alone).abs().max().item()
    print(f"packed vs alone: with doc_start {diff:.3e}, without {leak:.3e}")
    assert diff <= PACKED_VS_ALONE_BOUND, diff
    assert (also_a - a_alone).abs().max().item() <= PACKED_VS_ALONE_BOUND
    assert leak > 1000 * PACKED_VS_ALONE_BOUND, leak


def test_gradient_checkpointing_is_identical(tiny_llama_config):
    g = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (2, 64), generator=g)
    ds = dc.doc_start_from_lengths(([10, 54], [33, 1, 30]), 64)
    res = []
    for ckpt in (False, True):
        model = _tiny(tiny_llama_config).train()
        model.model.gradient_checkpointing = ckpt
        loss = model(input_ids=x, labels=x, doc_start=ds).loss
        loss.backward()
        res.append((loss.detach(), {n: p.grad for n, p in model.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys()
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n
    # and the mask is really on in both: the loss differs from the unmasked one
    plain = _tiny(tiny_llama_config).train()(input_ids=x, labels=x).loss
    assert abs(plain.item() - res[0][0].item()) > 1e-5


def test_doc_start_with_cache_raises(tiny_llama_config):
    from relora_amd.models.llama import LlamaForSequenceClassification

    model = _tiny(tiny_llama_config)
    x = torch.randint(0, 256, (1, 8))
    with torch.no_grad():
        past = model(input_ids=x, use_cache=True).past_key_values
    ds = torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="doc_start"):
        model(input_ids=x[:, :1], past_key_values=past, doc_start=ds)
    # the classification head passes doc_start down as well
    tiny_llama_config.num_labels = 2
    tiny_llama_config.pad_token_id = 0
    clf = LlamaForSequenceClassification(tiny_llama_config).eval()
    ds8 = dc.doc_start_from_lengths(([3, 5],), 8)
    with torch.no_grad():
        assert not torch.equal(clf(input_ids=x, doc_start=ds8).logits,
                               clf(input_ids=x).logits)


# ---- trainer ---------------------------------------------------------------

@pytest.fixture
def _single_proc_env(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    yield
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def _trainer_args(tmp_path, extra):
    from relora_amd.trainer import parse_args

    return parse_args([
        "--model_config", "configs/llama_9m.json", "--synthetic_data", "true",
        "--num_training_steps", "3", "--warmup_steps", "1",
        "--batch_size", "2", "--total_batch_size", "2", "--max_length", "32",
        "--lr", "1e-3", "--dtype", "float32", "--eval_every", "2", "--save_every", "100",
        "--workers", "0", "--save_dir", str(tmp_path / "run"),
    ] + extra)


def test_trainer_intra_doc_masking(tmp_path, monkeypatch, _single_proc_env):
    import torch.distributed as dist

    from relora_amd import trainer
    from relora_amd.data.dataloader import SyntheticDataset

    class Packed(SyntheticDataset):
        """random tokens with a separator (id 7) about every fifth token"""

        def __getitem__(self, idx):
            ids = super().__getitem__(idx)["input_ids"]
            g = torch.Generator().manual_seed(991 + idx)
            cut = torch.rand(ids.shape, generator=g) < 0.2
            return {"input_ids": torch.where(cut, torch.full_like(ids, 7), ids)}

    monkeypatch.setattr(trainer, "SyntheticDataset", Packed)
    seen = []
    real = ops.doc_starts_from_eos
    monkeypatch.setattr(ops, "doc_starts_from_eos",
                        lambda ids, sep: (seen.append(sep), real(ids, sep))[1])

    hist = []
    real_log = trainer.wandb.log
    monkeypatch.setattr(trainer.wandb, "log",
                        lambda m, **kw: (hist.append(dict(m)), real_log(m, **kw))[1])

    def losses(extra, sub):
        hist.clear()
        trainer.main(_trainer_args(tmp_path / sub, extra))
        if dist.is_initialized():
            dist.destroy_process_group()
        return [h["loss"] for h in hist if "loss" in h], \
               [h["final_eval_loss"] for h in hist if "final_eval_loss" in h]

    assert parse_default_is_off(tmp_path)
    off, off_eval = losses([], "off")
    assert not seen
    on, on_eval = losses(["--intra_doc_masking", "true", "--doc_separator_id", "7"], "on")
    assert seen and set(seen) == {7}
    assert len(seen) > 3, "evaluation batches must get doc_start too"
    assert len(on) == len(off) == 3
    assert all(x == x for x in on)
    assert on != off and on[0] != off[0], (on, off)
    assert on_eval and on_eval != off_eval
    # default separator: the model config's eos_token_id (no tokenizer here)
    seen.clear()
    losses(["--intra_doc_masking", "true"], "default_sep")
    assert set(seen) == {1}


def parse_default_is_off(tmp_path):
    args = _trainer_args(tmp_path / "d", [])
    return args.intra_doc_masking is False and args.doc_separator_id is None


def test_trainer_rejects_pythia_with_flag(tmp_path):
    from relora_amd.trainer import parse_args

    base = ["--model_config", "configs/pythia_160m.json", "--synthetic_data", "true",
            "--batch_size", "2", "--total_batch_size", "2", "--max_length", "32",
            "--dtype", "float32", "--save_dir", str(tmp_path / "run")]
    parse_args(base)   # Pythia alone is fine
    with pytest.raises(ValueError, match="intra_doc_masking"):
        parse_args(base + ["--intra_doc_masking", "true"])


# ---- conditioning of the GPU tests' inputs ---------------------------------

def test_gpu_inputs_are_well_conditioned():
    """On the exact inputs of tests/test_gpu_attention_docmask.py the masked
    bf16 emulation stays inside half of the project's bounds against the
    float64 reference, so a GPU failure is the kernel's.  Measured worst
    err/bound: o 0.17, dq 0.09, dk 0.39, dv 0.16; lse exact."""
    worst = {}
    for cid, nkv, S, hd, ds in dc.gpu_cases():
        assert dc.is_well_formed(ds), cid
        q, k, v, dout = dc.make_inputs(nkv, S, hd, ds)
        r = aw.all_ratios(dc.emulate_doc_bf16(q, k, v, dout, ds),
                          dc.ref_doc(q, k, v, dout, ds))
        for n, x in r.items():
            worst[n] = max(worst.get(n, 0.0), x)
        assert r.pop("lse") <= aw.LSE_TOL / 2 and max(r.values()) <= 0.5, (cid, r)
    print(f"docmask emulation worst err/bound: {worst}")
    # the two batch rows of every grid case differ
    for name in dc.GRID:
        ds = dc.grid_doc_start(name)
        assert not torch.equal(ds[0], ds[1]), name
    # q really alternates between 1x and Q_GAIN across a boundary
    ds = dc.grid_doc_start("mid45")
    q, _, _, _ = dc.make_inputs(4, dc.S_GRID, 64, ds)
    q0, _, _, _ = gc.make_inputs(dc.B, dc.NH, 4, dc.S_GRID, 64)
    assert torch.equal(q[0, :, :45], q0[0, :, :45])
    assert torch.equal(q[0, :, 45:].float(), q0[0, :, 45:].float() * dc.Q_GAIN)
