"""Constructions for the zero-point (AWQ) int4 tests: tests/w4a16_cases.py
with a zero-point added (positions, slicing and reporting come from
there), an AutoAWQ packer written from the format's description, and a
writer of a synthetic AWQ checkpoint directory.  The oracle is float64
``y[m, n] = sum_g s[n, g] * sum_{k in g} x[m, k] * (u[n, k] - z[n, g])``.
EXACT: ternary x, u and z uniform in 0..15, s = 2^a, a in -6..6: integer
group partials of the 128 + u form stay below 143 * sum|x| < 2^24 and all
values are multiples of 2^-6 below 2^18 (asserted), so ``torch.equal``.
NEEDLE: one +-1 per row, all 16 u, z per (n, g), distinct fp16 scales:
``bf16(+-s * (u - z))``, <= 11 + 5 significant bits, rounded once.
RANDOM: ``quantize_w4_zp`` weights, ``w4a16_cases.random_bound``'s form
with S = sum_g s sum_k |x| |u - z|.
"""

from __future__ import annotations

import json
import os
from typing import NamedTuple

import torch

from resilient_llm_amd.ops import ref

import w4a16_cases
from w4a16_cases import (BF16, GROUP, NNZ_MAX, SEED, _gen, needle_positions,
                         plan_slices)

AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


# ------------------------------------------------------------ AutoAWQ side
def _pack_cols(v: torch.Tensor) -> torch.Tensor:
    """[R, C] values 0..15 -> int32 [R, C/8]: nibble i of dword c holds
    column 8*c + AWQ_ORDER[i]."""
    v = v.to(torch.int64).reshape(v.shape[0], -1, 8)
    d = torch.zeros(v.shape[:2], dtype=torch.int64)
    for i, col in enumerate(AWQ_ORDER):
        d |= v[:, :, col] << (4 * i)
    return torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32)


def awq_pack(u: torch.Tensor, z: torch.Tensor, s: torch.Tensor):
    """(u [N, K], z [N, G], s fp16 [N, G]) -> (qweight int32 [K, N/8],
    qzeros int32 [G, N/8], scales fp16 [G, N]) as AutoAWQ stores them."""
    return (_pack_cols(u.t()), _pack_cols(z.t()),
            s.t().contiguous().to(torch.float16))


def write_awq_checkpoint(dense, path: str, **quantization_config) -> dict:
    """A directory like AutoAWQ's for a Llama: the unquantized model
    ``dense`` through ``quantize_w4_zp``, HF names, and a config.json whose
    quantization_config fields can be overridden.  Returns {fused
    projection: (packed, meta)} as a model holds them."""
    import safetensors.torch as st
    c = dense.config
    out, held = {}, {}
    parts = {"qkv": (("self_attn.q_proj", c.q_size),
                     ("self_attn.k_proj", c.kv_size),
                     ("self_attn.v_proj", c.kv_size)),
             "o": (("self_attn.o_proj", c.hidden_size),),
             "gate_up": (("mlp.gate_proj", c.intermediate_size),
                         ("mlp.up_proj", c.intermediate_size)),
             "down": (("mlp.down_proj", c.hidden_size),)}
    for i in range(c.n_layers):
        p = f"model.layers.{i}."
        for n, split in parts.items():
            u, z, s = ref.quantize_w4_zp(dense.params[f"l{i}.{n}"].cpu())
            held[f"l{i}.{n}"] = (ref.w4_pack(u.to(torch.int8) - 8),
                                 ref.w4_zp_meta(z, s))
            row = 0
            for hf, rows in split:
                sl = slice(row, row + rows)
                qw, qz, sc = awq_pack(u[sl], z[sl], s[sl])
                out[p + hf + ".qweight"] = qw
                out[p + hf + ".qzeros"] = qz
                out[p + hf + ".scales"] = sc
                row += rows
        out[p + "input_layernorm.weight"] = dense.params[f"l{i}.ln1"]
        out[p + "post_attention_layernorm.weight"] = dense.params[f"l{i}.ln2"]
    out["model.embed_tokens.weight"] = dense.params["embed"]
    out["model.norm.weight"] = dense.params["final_ln"]
    if dense.params["lm_head"] is not dense.params["embed"]:
        out["lm_head.weight"] = dense.params["lm_head"]
    os.makedirs(path, exist_ok=True)
    st.save_file({k: v.contiguous().cpu() for k, v in out.items()},
                 os.path.join(path, "model.safetensors"))
    qc = {"quant_method": "awq", "bits": 4, "group_size": 128,
          "version": "GEMM", "zero_point": True, **quantization_config}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "llama", "quantization_config": qc}, f)
    return held


# ------------------------------------------------------------------ oracle
def oracle64(x, u, z, s, absolute=False):
    """float64 [M, N] of the contract (``absolute``: of |x| and |u - z|)."""
    N, G = s.shape
    d = u.double().reshape(N, G, GROUP) - z.double().unsqueeze(-1)
    xd = x.double().reshape(-1, G, GROUP)
    if absolute:
        d, xd = d.abs(), xd.abs()
    part = torch.einsum("mgk,ngk->mng", xd, d)
    return (part * s.double().unsqueeze(0)).sum(dim=-1)


class Case(NamedTuple):
    name: str
    x: torch.Tensor           # [M, K] bf16
    u: torch.Tensor           # [N, K] uint8
    z: torch.Tensor           # [N, G] uint8
    s: torch.Tensor           # [N, G] fp16
    packed: torch.Tensor      # int32 [N*K/8]
    meta: torch.Tensor        # int32 [N, G]
    expected: torch.Tensor    # [M, N] bf16
    slices: list


def _case(name, x, u, z, s, expected, slices) -> Case:
    return Case(name, x, u, z, s, ref.w4_pack(u.to(torch.int8) - 8),
                ref.w4_zp_meta(z, s), expected, slices)


def exact_case(M, N, K, seed=SEED, slices=None) -> Case:
    g = _gen(seed + M + 3 * N + 7 * K)
    G = K // GROUP
    x = w4a16_cases.exact_case(M, N, K, seed).x.float()    # ternary rows
    assert int((x != 0).sum(dim=1).max()) <= NNZ_MAX
    u = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, G), generator=g, dtype=torch.uint8)
    a = torch.randint(-6, 7, (N, G), generator=g)
    s = torch.exp2(a.float()).to(torch.float16)
    assert torch.equal(s.float(), torch.exp2(a.float()))
    row_abs = int(x.abs().sum(dim=1).max())
    assert 143 * row_abs < 2 ** 24, row_abs        # integer group partials
    assert 64 * 15 * row_abs < 2 ** 18, row_abs    # multiples of 2^-6
    x = x.to(BF16)
    y = oracle64(x, u, z, s)
    assert torch.equal(y.float().double(), y)      # exact in f32
    return _case(f"exact M={M} N={N} K={K}", x, u, z, s, y.float().to(BF16),
                 slices or plan_slices(N, K))


def needle_weights(N, K, seed=SEED):
    """(u, z, s) shared by every sweep of one (N, K)."""
    g = _gen(seed + 11 * N + K)
    G = K // GROUP
    u = ((torch.arange(N)[:, None] * 5 + torch.arange(K)[None, :] * 3
          + torch.randint(0, 16, (1, K), generator=g)) % 16).to(torch.uint8)
    assert len(u.unique()) == 16
    z = ((torch.arange(N)[:, None] * 7 + torch.arange(G)[None, :] * 3
          + 1) % 16).to(torch.uint8)
    # consecutive fp16 bit patterns from 0x2400 (2^-6) up: N*G <= 8192
    # distinct positive normal values below 2^2, all 11 significant bits
    assert N * G <= 0x2000
    bits = (0x2400 + torch.randperm(N * G, generator=g)).to(torch.int16)
    s = bits.view(torch.float16).reshape(N, G).contiguous()
    assert len(s.float().unique()) == N * G
    return u, z, s


def needle_case(M, N, K, weights, sweep=0, seed=SEED, slices=None) -> Case:
    u, z, s = weights
    slices = slices or plan_slices(N, K)
    g = _gen(seed + 1 + sweep)
    pos = needle_positions(K, slices, seed)
    k_m = torch.tensor([pos[(sweep * M + m) % K] for m in range(M)])
    sign = torch.randint(0, 2, (M,), generator=g) * 2 - 1
    x = torch.zeros(M, K)
    x[torch.arange(M), k_m] = sign.float()
    x = x.to(BF16)
    g_m = k_m // GROUP
    closed = (s[:, g_m].float() * (u[:, k_m].float() - z[:, g_m].float())).T \
        * sign[:, None].float()
    expected = closed.to(BF16)
    assert torch.equal(oracle64(x, u, z, s).float().to(BF16), expected)
    return _case(f"needle M={M} N={N} K={K} sweep={sweep} k_m="
                 f"{k_m.tolist()[:12]}", x, u, z, s, expected, slices)


def random_case(M, N, K, seed=SEED) -> Case:
    g = _gen(seed + 2 + M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (0.02 * torch.randn(N, K, generator=g)).to(BF16)
    u, z, s = ref.quantize_w4_zp(w)
    y = oracle64(x, u, z, s)
    return _case(f"random M={M} N={N} K={K}", x, u, z, s, y.float().to(BF16),
                 plan_slices(N, K))


def random_bound(case: Case):
    """(y64, allowed |got - y64|, S) of a RANDOM case, float64 [M, N]:
    ``w4a16_cases.random_bound`` with S = sum_g s sum_k |x| |u - z|."""
    y = oracle64(case.x, case.u, case.z, case.s)
    S = oracle64(case.x, case.u, case.z, case.s, absolute=True)
    return y, 2.0 ** -8 * y.abs() + 2.0 ** -19 * S, S


def layer_case(N, K, seed=SEED):
    """Random (u, z, s) with any normal fp16 scale in 2^-12 .. 2^12 and
    the closed-form dequantized weight bf16 [N, K]."""
    g = _gen(seed + 5 + N + K)
    G = K // GROUP
    u = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, G), generator=g, dtype=torch.uint8)
    s = (torch.exp2(torch.randint(-12, 13, (N, G), generator=g).float())
         * (1 + torch.rand(N, G, generator=g))).to(torch.float16)
    w = (s.float().repeat_interleave(GROUP, dim=1)
         * (u.float() - z.float().repeat_interleave(GROUP, dim=1))).to(BF16)
    return u, z, s, w
