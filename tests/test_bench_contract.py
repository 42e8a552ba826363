"""bench.py driver contract: one JSON line on stdout (rank 0) with the
fields the round driver parses, runnable end-to-end on CPU with a tiny
model (the GPU run only changes device/dtype, not the contract)."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _run_bench(*extra):
    env = {**os.environ, "PYTHONPATH": REPO, "RELORA_AMD_NO_TQDM": "1"}
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--model", "configs/llama_9m.json", "--steps", "2", "--warmup", "1",
         "--batch_size", "2", "--seq_len", "32", "--dtype", "fp32",
         "--lora_r", "8", *extra],
        capture_output=True, text=True, env=env, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_bench_json_contract(tmp_path):
    r = _run_bench()
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1, r.stdout[-2000:]
    out = json.loads(json_lines[0])

    assert REQUIRED <= set(out), REQUIRED - set(out)
    assert out["n_gpus"] == 1
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["unit"] == "tokens/s"
    cfg = out["config"]
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in cfg, k
    assert cfg["parallelism"] == "dp1"
    assert cfg["global_batch"] == 2 and cfg["seq_len"] == 32
    # whole-job aggregate: value * elapsed == tokens processed
    tokens = cfg["global_batch"] * cfg["seq_len"] * out["steps"]
    elapsed_s = out["ms_per_step"] * out["steps"] / 1000
    assert abs(out["value"] - tokens / elapsed_s) / out["value"] < 1e-6


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's loss and (sampled)
    trainable parameters as float32 .npy; the same arguments give the same
    inputs, so two runs of one build write the same arrays."""
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _run_bench("--dump-outputs", str(d))
        out = json.loads([l for l in r.stdout.splitlines()
                          if l.startswith("{")][-1])
        assert sorted(os.listdir(d)) == ["loss.npy", "params.npy"]
        arrays = {n: np.load(d / f"{n}.npy") for n in ("loss", "params")}
        for a in arrays.values():
            assert a.dtype == np.float32 and np.isfinite(a).all()
        assert arrays["loss"].shape == (1,)
        assert abs(float(arrays["loss"][0]) - out["config"]["final_loss"]) < 1e-3
        assert arrays["params"].ndim == 1 and arrays["params"].size > 0
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
        dumps.append(arrays)
    for n in ("loss", "params"):
        np.testing.assert_array_equal(dumps[0][n], dumps[1][n])
