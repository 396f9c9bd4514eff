"""Qwen3 q/k norm on the CPU: the reference ops against a direct float64
formula, the tiny-qk model through prefill / decode / the engine, and the
checkpoint round trip with its two mismatch errors."""

import dataclasses

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref
from qk_norm_cases import norm_rope64


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


@pytest.mark.parametrize("D", [64, 128])
def test_ref_ops_against_float64(D):
    g = torch.Generator().manual_seed(D)
    T, n_q, n_kv, bs, eps = 5, 4, 2, 16, 1e-6
    qkv = torch.randn(T, (n_q + 2 * n_kv) * D, generator=g)
    wq = 1 + 0.25 * torch.randn(D, generator=g)
    wk = 1 + 0.25 * torch.randn(D, generator=g)
    pos = _i32([0, 3, 7, 8, 30])
    slots = _i32([16, 17, -1, 2, 40])
    cs = ref.build_cos_sin(64, D)
    kc = torch.full((3, n_kv, bs, D), float("nan"))
    vc = torch.full_like(kc, float("nan"))
    q0, k0, v0 = (t.reshape(T, -1, D).clone() for t in
                  qkv.split([n_q * D, n_kv * D, n_kv * D], dim=1))
    x = qkv.clone()
    ops.qk_norm_rope_kv_append_qkv_(x, wq, wk, eps, pos, cs, kc, vc, slots,
                                    n_q)
    _, q_want = norm_rope64(q0, wq, eps, pos, cs)
    _, k_want = norm_rope64(k0, wk, eps, pos, cs)
    q, k, v = (t.reshape(T, -1, D) for t in
               x.split([n_q * D, n_kv * D, n_kv * D], dim=1))
    torch.testing.assert_close(q.double(), q_want, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(k.double(), k_want, atol=1e-5, rtol=1e-5)
    assert torch.equal(v, v0)
    written = torch.zeros(3 * bs, dtype=torch.bool)
    for t, s in enumerate(slots.tolist()):
        if s < 0:
            continue
        written[s] = True
        assert torch.equal(kc[s // bs, :, s % bs], k[t])
        assert torch.equal(vc[s // bs, :, s % bs], v0[t])
    # nothing else was touched
    assert torch.isnan(kc.transpose(1, 2).reshape(3 * bs, -1)[~written]).all()


def _model(name, seed=3):
    cfg = get_config(name)
    m = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for i in range(cfg.n_layers):
        for n in ("q_norm", "k_norm"):
            if cfg.qk_norm:
                m.params[f"l{i}.{n}"] = 1 + 0.25 * torch.randn(
                    cfg.head_dim, generator=g)
    return cfg, m


def _kv(cfg, nb):
    kv = PagedKVCache.for_model(cfg, nb, device="cpu")
    kv.k, kv.v = kv.k.float(), kv.v.float()
    return kv


def test_tiny_qk_decode_matches_prefill():
    cfg, m = _model("tiny-qk")
    assert cfg.q_size != cfg.hidden_size
    p = 21
    ids = [(5 * t + 1) % cfg.vocab_size for t in range(p + 1)]
    full = m.forward_prefill(_i32(ids), _i32(list(range(p + 1))), _kv(cfg, 4),
                             _i32(list(range(p + 1))), _i32([0, p + 1]))
    kv = _kv(cfg, 4)
    m.forward_prefill(_i32(ids[:p]), _i32(list(range(p))), kv,
                      _i32(list(range(p))), _i32([0, p]))
    dec = m.forward_decode(_i32(ids[p:]), _i32([p]), kv, _i32([p]),
                           _i32([[0, 1]]), _i32([p + 1]))
    torch.testing.assert_close(dec, full, atol=1e-4, rtol=1e-4)
    # the norm weights take part: with ones the logits move
    for i in range(cfg.n_layers):
        m.params[f"l{i}.k_norm"] = torch.ones(cfg.head_dim)
    moved = m.forward_prefill(_i32(ids), _i32(list(range(p + 1))),
                              _kv(cfg, 4), _i32(list(range(p + 1))),
                              _i32([0, p + 1]))
    assert (moved - full).abs().max() > 1e-3


def test_checkpoint_round_trip_and_mismatches(tmp_path):
    cfg, m = _model("tiny-qk")
    path = str(tmp_path / "qk")
    m.save_safetensors(path)
    twin = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=9)
    twin.load_safetensors(path)
    for i in range(cfg.n_layers):
        for n in ("q_norm", "k_norm"):
            assert torch.equal(twin.params[f"l{i}.{n}"], m.params[f"l{i}.{n}"])
    # the same geometry without the norm: the keys would be dropped
    plain_cfg = dataclasses.replace(cfg, name="tiny-plain", qk_norm=False)
    plain = LlamaForCausalLM(plain_cfg, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.k_norm"):
        plain.load_safetensors(path)
    # and the reverse: a checkpoint without them into a q/k-norm model
    path2 = str(tmp_path / "plain")
    plain.save_safetensors(path2)
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_norm"):
        twin.load_safetensors(path2)


def test_engine_on_tiny_qk_frees_every_block():
    cfg, m = _model("tiny-qk")
    kv = _kv(cfg, 32)
    free0 = kv.free_blocks
    e = LLMEngine(m, kv, max_batch_size=4)
    for r in range(3):
        e.add_request(f"r{r}", list(range(3 + r, 30 + 3 * r)),
                      SamplingParams(max_tokens=6, temperature=0.0))
    n = 0
    while e.has_work():
        n += len(e.step())
    assert n == 18
    assert kv.free_blocks == free0


def test_qwen3_presets():
    c = get_config("qwen3-8b")
    assert c.qk_norm and c.q_size == 4096 and c.head_dim == 128
    assert get_config("qwen3-32b").q_size != get_config("qwen3-32b").hidden_size
    assert get_config("qwen3-0.6b").tie_embeddings
