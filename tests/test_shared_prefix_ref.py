"""Shared-prefix decode attention without a GPU: the host plan builder on
hand-written block lists, the engine option on the CPU reference ops, and
the option's validation and way to the worker's command line."""

import pytest
from resilient_llm_amd.config import ConfigError, load_config
from resilient_llm_amd.engine import SamplingParams
from resilient_llm_amd.engine.kv_cache import shared_prefix_groups
from tests.test_engine import drain, make_engine, tokens_of


def test_two_groups_and_a_loner_interleaved():
    lists = [[3, 4, 10, 11],        # group A
             [7, 8, 20],            # group B
             [3, 4, 12],            # A
             [30, 31],              # loner
             [7, 8, 21, 22],        # B
             [3, 4, 13]]            # A
    cached = [50, 40, 47, 20, 60, 33]
    p = shared_prefix_groups(lists, cached, 16, 32, 16)
    assert p["n_shared"] == [32, 32, 32, 0, 32, 32]
    assert p["row_tile"] == [0, 1, 0, -1, 1, 0]
    assert p["row_slot"] == [0, 0, 1, 0, 1, 2]
    assert p["tile_rows"] == [[0, 2, 5] + [-1] * 13, [1, 4] + [-1] * 14]
    assert p["tile_blocks"] == [2, 2]
    assert p["tile_bt_row"] == [0, 1]


def test_clamp_threshold_and_tiles():
    same = [[1, 2, 3, 9], [1, 2, 3, 8]]
    # the third common block is not full for the row with 40 cached tokens
    assert shared_prefix_groups(same, [60, 40], 16, 16, 16)["tile_blocks"] == [2]
    assert shared_prefix_groups(same, [60, 48], 16, 16, 16)["tile_blocks"] == [3]
    # two shared blocks are 32 tokens: below a threshold of 33 no group forms
    assert shared_prefix_groups(same, [60, 40], 16, 33, 16) is None
    assert shared_prefix_groups([[1, 2], [3, 4]], [32, 32], 16, 16, 16) is None
    # 9 members at 8 per tile spill into a second tile
    p = shared_prefix_groups([[5, 6, 100 + i] for i in range(9)], [33] * 9,
                             16, 16, 8)
    assert p["tile_rows"] == [list(range(8)), [8] + [-1] * 7]
    assert p["tile_blocks"] == [2, 2] and p["tile_bt_row"] == [0, 8]
    assert p["row_tile"] == [0] * 8 + [1] and p["row_slot"][8] == 0


def test_engine_group_emits_the_same_tokens_with_the_option_on():
    def run(**kw):
        e = make_engine(num_blocks=64, max_batch_size=4, **kw)
        rids = [f"g.c{i}" for i in range(4)]
        e.add_request_group(rids, [5 + (7 * i) % 90 for i in range(40)],
                            [SamplingParams(max_tokens=10, temperature=0.8,
                                            seed=50 + i, stop_on_eos=False)
                             for i in range(4)])
        outs = drain(e)
        assert e.kv.free_blocks == e.kv.num_blocks
        return [tokens_of(outs, r) for r in rids], e.stats

    off, stats_off = run()
    on, stats_on = run(shared_prefix_attention=True,
                       shared_prefix_min_tokens=16)
    assert on == off and all(len(t) == 10 for t in on)
    assert stats_off["shared_prefix_steps"] == 0
    assert stats_on["shared_prefix_steps"] > 0
    assert stats_on["shared_prefix_rows"] == 4 * stats_on["shared_prefix_steps"]
    # at the default threshold a 40-token prompt forms no group
    _, stats_default = run(shared_prefix_attention=True)
    assert stats_default["shared_prefix_steps"] == 0


def _config(model, **params):
    return {"cluster": {"pools": {"p0": {"gpus": [0, 1],
                                         "tensor_parallel": 2}}},
            "model_list": [{"model_name": "m", "litellm_params":
                            {"model": model, **params}}]}


@pytest.mark.parametrize("model,params", [
    ("gpu/0/tiny", {"shared_prefix_attention": "yes"}),
    ("gpu/0/tiny", {"shared_prefix_attention": 1}),
    ("gpu/0/tiny", {"shared_prefix_attention": True, "kv_dtype": "fp8"}),
    ("pool/p0/tiny", {"shared_prefix_attention": True}),
    ("gpu/0/tiny", {"shared_prefix_min_tokens": 8}),
    ("gpu/0/tiny", {"shared_prefix_min_tokens": "1024"}),
])
def test_config_rejects(model, params):
    with pytest.raises(ConfigError, match="shared_prefix"):
        load_config(data=_config(model, **params))


def test_config_accepts_and_worker_command_line_carries_it(monkeypatch):
    cfg = load_config(data=_config("gpu/0/tiny", shared_prefix_attention=True,
                                   shared_prefix_min_tokens=2048,
                                   quantization="int4"))
    assert cfg.deployments[0].params["shared_prefix_min_tokens"] == 2048
    from resilient_llm_amd.workers import gpu
    cmds = []
    monkeypatch.setattr(gpu.subprocess, "Popen",
                        lambda cmd, env=None: cmds.append(cmd))
    gpu.spawn_gpu_worker("0", "tiny", "/tmp/x.sock",
                         shared_prefix_attention=True,
                         shared_prefix_min_tokens=2048)
    gpu.spawn_gpu_worker("0", "tiny", "/tmp/x.sock")
    i = cmds[0].index("--shared-prefix-min-tokens")
    assert "--shared-prefix-attention" in cmds[0] and cmds[0][i + 1] == "2048"
    assert "--shared-prefix-attention" not in cmds[1]
