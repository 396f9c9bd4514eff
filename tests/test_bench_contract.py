"""bench.py driver contract: run the flagship bench on CPU (tiny model,
1 step, low concurrency) and validate the single JSON line it prints —
every field the driver/judge parses must be present and well-typed.
Catches regressions to the contract before they reach a GPU run."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.timeout(300)


def test_bench_dump_is_reproducible(tmp_path):
    """Same arguments -> same prompts -> same dumped token ids, row for
    row, whatever order the requests arrived in."""
    import numpy as np
    dumps = []
    for name in ("a", "b"):
        proc = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"),
             "--steps", "2", "--warmup", "1", "--model", "tiny",
             "--concurrency", "4", "--prompt-tokens", "16",
             "--output-tokens", "8", "--device", "cpu",
             "--dump-outputs", str(tmp_path / name)],
            capture_output=True, text=True, timeout=280, cwd=REPO)
        assert proc.returncode == 0, proc.stderr[-2000:]
        dumps.append(np.load(tmp_path / name / "token_ids.npy"))
    assert dumps[0].shape == (4, 8)
    assert np.array_equal(dumps[0], dumps[1])
    # four different prompts: the rows are not all one completion
    assert len({tuple(r) for r in dumps[0]}) > 1


def test_bench_json_contract(tmp_path):
    dump = tmp_path / "outputs"
    proc = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--steps", "1", "--warmup", "0", "--model", "tiny",
         "--concurrency", "4", "--prompt-tokens", "16",
         "--output-tokens", "8", "--device", "cpu",
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=280, cwd=REPO)
    assert proc.returncode == 0, proc.stderr[-2000:]
    # a plain run reports nothing beyond the headline (that is --full)
    assert "engine stats" not in proc.stderr

    # --dump-outputs: one row of token ids per request of the last step
    import numpy as np
    assert sorted(os.listdir(dump)) == ["completion_tokens.npy",
                                        "token_ids.npy"]
    toks = np.load(dump / "token_ids.npy")
    n_out = np.load(dump / "completion_tokens.npy")
    assert toks.dtype == np.float32 and toks.shape == (4, 8)
    assert n_out.dtype == np.float32 and n_out.shape == (4,)
    assert ((n_out >= 1) & (n_out <= 8)).all()
    for row, n in zip(toks, n_out.astype(int)):
        assert ((row[:n] >= 0) & (row[:n] < 512)).all()   # tiny vocab
        assert (row[:n] == np.round(row[:n])).all()
        assert (row[n:] == -1).all()

    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    out = json.loads(lines[0])

    # metric string is BASELINE.json's, verbatim
    assert out["metric"] == ("sustained reqs/sec + success-rate + "
                             "p50 latency @ 64 concurrent, Llama-3-8B")
    assert isinstance(out["value"], (int, float)) and out["value"] > 0
    assert out["unit"] == "reqs/s"
    assert out["n_gpus"] == 1
    assert out["steps"] == 1
    assert out["warmup"] == 0
    assert isinstance(out["ms_per_step"], (int, float)) and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["dtype"] == "bf16"
    assert out["data"] == "synthetic"
    # vs_baseline: number or null (BASELINE.md has no native-hw number)
    assert out["vs_baseline"] is None or isinstance(out["vs_baseline"], (int, float))
    cfg = out["config"]
    assert cfg["model"] == "tiny"
    assert cfg["concurrency_per_gpu"] == 4
    assert cfg["global_batch"] == 4
    assert cfg["parallelism"] == "dp1"
    assert cfg["success_rate"] == 1.0
    assert cfg["p50_latency_s"] > 0
    assert cfg["p99_latency_s"] >= cfg["p50_latency_s"]
    assert cfg["output_tokens_per_s"] > 0
    assert cfg["total_tokens_per_s"] > cfg["output_tokens_per_s"]
