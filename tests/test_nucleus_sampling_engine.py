"""The engine's device_sampling mode on the CPU reference ops, and the
option's way from the config to the worker's command line."""

from collections import Counter

import pytest
from resilient_llm_amd import ops
from resilient_llm_amd.config import ConfigError, load_config
from resilient_llm_amd.engine import SamplingParams
from tests.test_engine import drain, make_engine, tokens_of

PROMPT = [7, 8, 9, 10]


def engine(**kw):
    return make_engine(num_blocks=600, model_seed=3, max_batch_size=4,
                       max_model_len=8192, **kw)


def sp(**kw):
    return SamplingParams(stop_on_eos=False, **kw)


def test_routing_and_history_across_a_rebuild(monkeypatch):
    """Never _sample_torch; a request joins mid-decode, and every history
    the op is handed equals the row's output_ids at that step."""
    e = engine(device_sampling=True)
    monkeypatch.setattr(e, "_sample_torch", lambda *a, **k: pytest.fail(
        "_sample_torch reached"))
    real, seen = ops.sample_nucleus, []

    def checked(logits, rows, *rest, **kw):
        if logits.shape[0] == len(e.running):             # a decode step
            for row, slot in zip(rows.tolist(), rest[-4].tolist()):
                if slot >= 0:
                    n = int(rest[-2][slot])
                    assert rest[-3][slot, :n].tolist() \
                        == e.running[row].output_ids
                    seen.append(e.running[row].req_id)
        return real(logits, rows, *rest, **kw)

    monkeypatch.setattr(ops, "sample_nucleus", checked)
    e.add_request("pen", PROMPT, sp(max_tokens=16, frequency_penalty=0.5,
                                    presence_penalty=0.25))
    e.add_request("p", PROMPT, sp(max_tokens=16, temperature=0.8, top_p=0.7,
                                  seed=5))
    for _ in range(6):
        e.step()
    e.add_request("late", PROMPT, sp(max_tokens=8, temperature=1.0, seed=2,
                                     presence_penalty=0.5))
    assert len(drain(e)["late"]) == 8
    assert seen.count("pen") >= 12 and seen.count("late") >= 5
    assert not e._b_torch_sampling


def test_a_penalty_row_over_the_history_cap_keeps_the_torch_path(monkeypatch):
    e = engine(device_sampling=True)
    reached = []
    real = e._sample_torch
    monkeypatch.setattr(e, "_sample_torch",
                        lambda lg, s: reached.append(s.req_id) or real(lg, s))
    cap = ops.sample_nucleus_max_history()
    e.add_request("big", PROMPT, sp(max_tokens=cap + 1, presence_penalty=0.5))
    e.add_request("p", PROMPT, sp(max_tokens=cap + 1, temperature=0.8,
                                  top_p=0.7, seed=5))     # no history: device
    for _ in range(4):
        e.step()
    assert set(reached) == {"big"}


def test_frequency_penalty_reduces_repetition():
    def run(pen):
        e = engine(device_sampling=True)
        e.add_request("a", PROMPT, sp(max_tokens=24, frequency_penalty=pen))
        return tokens_of(drain(e), "a")

    base, pen = run(0.0), run(50.0)
    assert len(pen) == len(base) == 24
    top = lambda ts: max(Counter(ts).values())   # noqa: E731
    assert top(pen) < top(base) or top(base) == 1


def test_option_off_never_calls_the_op(monkeypatch):
    monkeypatch.setattr(ops, "sample_nucleus", lambda *a, **k: pytest.fail(
        "sample_nucleus called"))
    e = engine()
    e.add_request("p", PROMPT, sp(max_tokens=6, temperature=0.8, top_p=0.7,
                                  seed=5, frequency_penalty=0.5))
    assert len(drain(e)["p"]) == 6 and e._b_torch_sampling


def _config(model, **params):
    return {"cluster": {"pools": {"p0": {"gpus": [0, 1],
                                         "tensor_parallel": 2}}},
            "model_list": [{"model_name": "m", "litellm_params":
                            {"model": model, **params}}]}


def test_config_validates_the_option():
    cfg = load_config(data=_config("gpu/0/tiny", device_sampling=True))
    assert cfg.deployments[0].params["device_sampling"] is True
    for bad in ("yes", 1, None):
        with pytest.raises(ConfigError):
            load_config(data=_config("gpu/0/tiny", device_sampling=bad))
    with pytest.raises(ConfigError):
        load_config(data=_config("pool/p0/tiny", device_sampling=True))


def test_worker_command_line_carries_the_flag(monkeypatch):
    from resilient_llm_amd.workers import gpu
    cmds = []
    monkeypatch.setattr(gpu.subprocess, "Popen",
                        lambda cmd, env=None: cmds.append(cmd))
    gpu.spawn_gpu_worker("0", "tiny", "/tmp/x.sock", device_sampling=True)
    gpu.spawn_gpu_worker("0", "tiny", "/tmp/x.sock")
    assert "--device-sampling" in cmds[0]
    assert "--device-sampling" not in cmds[1]
