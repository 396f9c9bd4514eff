"""Llama-family model, MI355X-first.

No nn.Module graph: a flat parameter store + an explicit forward written
against the serving ops — fused QKV / gate-up GEMMs through hipBLASLt
(torch.nn.functional.linear), everything between the GEMMs as hand-written
gfx950 kernels (resilient_llm_amd.ops): fused residual-add RMSNorm,
RoPE+paged-KV append, paged GQA decode attention, varlen prefill
attention, fused SwiGLU.  On CPU the same forward runs on the fp32
reference ops — that is the no-GPU test path.

The reference runs no model code at all (model execution lives inside
AWS Bedrock — SURVEY.md §0); targets here come from BASELINE.json:
Llama-3-8B bf16 as the flagship, Llama-3-70B TP=4 per pool.

Weight loading: random init (no-network default) or a safetensors
directory with HF Llama names.
"""

from __future__ import annotations

import dataclasses
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import autotune as lt_autotune

# Opt-in: route decode-shaped GEMMs (M<=64) through the custom skinny-M
# MFMA kernel instead of hipBLASLt (A/B lever; see ops/csrc/skinny_gemm.hip)
_USE_SKINNY = os.environ.get("RLLI_SKINNY") == "1"


# Row counts that the measured-GEMM autotuner may tune: the decode graph
# buckets (+ the small row counts prefill's lm_head sees).  Anything else
# (prefill/mixed token counts — unbounded variety) goes straight to
# torch so the tuning cache stays finite.
_LT_ROWS = frozenset({1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128})


def _linear(x, w):
    if _USE_SKINNY:
        return ops.linear_auto(x, w)
    if x.is_cuda and x.dim() == 2 and x.shape[0] in _LT_ROWS:
        return lt_autotune.tuned_linear(x, w)
    return F.linear(x, w)


@dataclasses.dataclass
class LlamaConfig:
    name: str
    hidden_size: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    head_dim: int
    intermediate_size: int
    vocab_size: int
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    # token ids that end generation (Llama-3: <|end_of_text|>=128001 and
    # <|eot_id|>=128009); overridable per deployment / by a real tokenizer
    eos_ids: tuple = (2,)
    # Qwen3: a per-head RMSNorm on q and on k (weights [head_dim], shared by
    # all heads) between the qkv projection and RoPE
    qk_norm: bool = False
    # Qwen3-MoE: every layer's MLP is num_experts SwiGLU experts of width
    # moe_intermediate_size, experts_per_token of them run per token,
    # weighted by a softmax-top-k router (norm_topk_prob: the chosen
    # weights are renormalised to sum to 1).  0 experts: the dense MLP.
    num_experts: int = 0
    experts_per_token: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = True

    @property
    def q_size(self) -> int:
        return self.n_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.n_kv_heads * self.head_dim


MODEL_PRESETS: dict[str, LlamaConfig] = {
    "llama-3-8b": LlamaConfig(
        name="llama-3-8b", hidden_size=4096, n_layers=32, n_heads=32,
        n_kv_heads=8, head_dim=128, intermediate_size=14336,
        vocab_size=128256, eos_ids=(128001, 128009)),
    "llama-3-70b": LlamaConfig(
        name="llama-3-70b", hidden_size=8192, n_layers=80, n_heads=64,
        n_kv_heads=8, head_dim=128, intermediate_size=28672,
        vocab_size=128256, eos_ids=(128001, 128009)),
    "llama-3-1b": LlamaConfig(
        # Llama-3.2-1B geometry: small-footprint replica for dense
        # multi-replica serving on one GPU (head_dim 64 path)
        name="llama-3-1b", hidden_size=2048, n_layers=16, n_heads=32,
        n_kv_heads=8, head_dim=64, intermediate_size=8192,
        vocab_size=128256, eos_ids=(128001, 128009)),
    "mistral-7b": LlamaConfig(
        # Mistral-7B-v0.3 geometry (no sliding window: full attention,
        # which is exact for contexts <= max_position)
        name="mistral-7b", hidden_size=4096, n_layers=32, n_heads=32,
        n_kv_heads=8, head_dim=128, intermediate_size=14336,
        vocab_size=32768, rope_theta=1000000.0),
    # Qwen3 dense family: q/k norm, head_dim independent of hidden_size /
    # n_heads, tied embeddings at the small sizes.  Geometry written from
    # memory of the published config.json files - no checkpoint was at hand
    # to check it against; load_safetensors' shape checks make a wrong
    # number fail at load.
    "qwen3-0.6b": LlamaConfig(
        name="qwen3-0.6b", hidden_size=1024, n_layers=28, n_heads=16,
        n_kv_heads=8, head_dim=128, intermediate_size=3072,
        vocab_size=151936, rope_theta=1000000.0, rms_eps=1e-6,
        max_position=40960, tie_embeddings=True,
        eos_ids=(151645, 151643), qk_norm=True),
    "qwen3-8b": LlamaConfig(
        name="qwen3-8b", hidden_size=4096, n_layers=36, n_heads=32,
        n_kv_heads=8, head_dim=128, intermediate_size=12288,
        vocab_size=151936, rope_theta=1000000.0, rms_eps=1e-6,
        max_position=40960, eos_ids=(151645, 151643), qk_norm=True),
    "qwen3-32b": LlamaConfig(
        name="qwen3-32b", hidden_size=5120, n_layers=64, n_heads=64,
        n_kv_heads=8, head_dim=128, intermediate_size=25600,
        vocab_size=151936, rope_theta=1000000.0, rms_eps=1e-6,
        max_position=40960, eos_ids=(151645, 151643), qk_norm=True),
    # Qwen3-MoE: qwen3-8b's attention side at hidden 2048 and a sparse MLP
    # in every layer, no shared expert.  As above the geometry is written
    # from memory of the published config.json, and load_safetensors' shape
    # checks are what catches a wrong number.
    "qwen3-30b-a3b": LlamaConfig(
        name="qwen3-30b-a3b", hidden_size=2048, n_layers=48, n_heads=32,
        n_kv_heads=4, head_dim=128, intermediate_size=6144,
        vocab_size=151936, rope_theta=1000000.0, rms_eps=1e-6,
        max_position=40960, eos_ids=(151645, 151643), qk_norm=True,
        num_experts=128, experts_per_token=8, moe_intermediate_size=768,
        norm_topk_prob=True),
    # CPU-testable models
    "tiny-moe": LlamaConfig(
        name="tiny-moe", hidden_size=256, n_layers=2, n_heads=4,
        n_kv_heads=2, head_dim=64, intermediate_size=512, vocab_size=512,
        max_position=2048, qk_norm=True, num_experts=8,
        experts_per_token=2, moe_intermediate_size=128),
    "tiny": LlamaConfig(
        name="tiny", hidden_size=256, n_layers=2, n_heads=4, n_kv_heads=2,
        head_dim=64, intermediate_size=512, vocab_size=512,
        max_position=2048),
    "tiny-128": LlamaConfig(
        name="tiny-128", hidden_size=512, n_layers=2, n_heads=4, n_kv_heads=1,
        head_dim=128, intermediate_size=1024, vocab_size=512,
        max_position=2048),
    # q/k-norm forms of the two above; tiny-qk has q_size (512) != hidden
    "tiny-qk": LlamaConfig(
        name="tiny-qk", hidden_size=256, n_layers=2, n_heads=8, n_kv_heads=2,
        head_dim=64, intermediate_size=512, vocab_size=512,
        max_position=2048, qk_norm=True),
    "tiny-qk-128": LlamaConfig(
        name="tiny-qk-128", hidden_size=512, n_layers=2, n_heads=4,
        n_kv_heads=1, head_dim=128, intermediate_size=1024, vocab_size=512,
        max_position=2048, qk_norm=True),
}


def get_config(name: str) -> LlamaConfig:
    try:
        return MODEL_PRESETS[name]
    except KeyError:
        raise KeyError(f"unknown model {name!r}; have {sorted(MODEL_PRESETS)}")


class LlamaForCausalLM:
    """Inference-only Llama.  TP sharding plugs in via `shard` (see
    resilient_llm_amd.parallel): rank/world split q/kv heads and the
    intermediate dim column-wise, o/down row-wise, with an all-reduce
    after o_proj and down_proj."""

    def __init__(self, config: LlamaConfig, device: str = "cpu",
                 dtype: torch.dtype = torch.bfloat16,
                 tp_rank: int = 0, tp_world: int = 1,
                 tp_group=None, seed: int = 0,
                 quant: Optional[str] = None) -> None:
        self.config = config
        self.device = torch.device(device)
        self.dtype = dtype
        # quant="fp8": W8A8-fp8 for the three bandwidth-dominant
        # projections (gate_up, down, lm_head) — per-out-channel weight
        # scales + per-row dynamic activation scales emitted by the
        # fused rmsnorm/silu kernels, rowwise torch._scaled_mm compute
        # (hipBLASLt fp8 MFMA).  qkv/o stay bf16: measured 1.0x in fp8
        # at decode shapes (ramp-bound), so quantizing them buys
        # nothing and costs an attention-output quantization step.
        # quant="int4": W4A16 for the four layer projections (qkv, o,
        # gate_up, down) — symmetric group-128 int4 weights, quantized
        # round-to-nearest at load, bf16 activations; lm_head, embed and
        # the norms stay bf16.  Up to 64 rows run the fused HIP GEMM
        # (ops.w4a16_linear), 65..256 rows its tiled form
        # (ops.w4a16_tiled_linear: the decode batches the graph buckets
        # go up to, mixed chunked-prefill and spec_lookup steps; a shape
        # measured slower there stops lower, _W4_TILED_ROWS_BY_SHAPE); the
        # shapes and rows of _W4_WIDE_ROWS_BY_SHAPE, up to 512, run the
        # wide form (ops.w4a16_wide_linear) in those steps instead; more
        # rows dequantize one projection at a time into a shared scratch
        # buffer and take the bf16 GEMM.  So does every whole-prompt
        # prefill step (forward_prefill) above 64 rows, as it always did:
        # the tiled form is the path of decode, mixed and verification
        # steps, and what prefill computes stays what it was.
        # quant="int4-awq": the int4 path with a per-group zero-point and fp16
        # scales (ops.w4a16_zp_linear / ops.w4a16_zp_tiled_linear /
        # ops.w4_zp_dequant, routed by rows in the same way), the form
        # AutoAWQ checkpoints hold: load_safetensors repacks their
        # tensors on the device (ops.awq_repack); random init quantizes
        # asymmetric min/max round-to-nearest.  (A mode of the int4 path,
        # hence the name; a bare "awq" stays an unknown value.)
        if quant not in (None, "fp8", "int4", "int4-awq"):
            raise ValueError(f"quant must be None, 'fp8', 'int4' or "
                             f"'int4-awq', got {quant!r}")
        if (quant in ("int4", "int4-awq")
                and torch.device(device).type == "cuda"
                and dtype != torch.bfloat16):
            raise ValueError(f"quant={quant!r} on a GPU needs dtype bfloat16 "
                             f"(the fused kernel reads bf16 activations), "
                             f"got {dtype}")
        if quant == "int4-awq" and tp_world > 1:
            raise ValueError("quant='int4-awq' does not shard: "
                             "tensor_parallel must be 1")
        # Mixture-of-Experts configs (num_experts > 0): bf16 experts on one
        # GPU, routed by ops.moe_route and run by ops.moe_mlp in every step
        # (prefill, mixed, decode and the captured graph alike)
        if config.num_experts:
            if quant is not None:
                raise ValueError(f"{config.name} is a Mixture-of-Experts "
                                 f"model: quant must be None, got {quant!r}")
            if tp_world > 1:
                raise ValueError(f"{config.name} is a Mixture-of-Experts "
                                 f"model: tensor_parallel must be 1")
        self.quant = quant
        self.tp_rank = tp_rank
        self.tp_world = tp_world
        self.tp_group = tp_group
        c = config
        assert c.n_heads % tp_world == 0 and c.n_kv_heads % tp_world == 0, \
            f"TP={tp_world} must divide heads ({c.n_heads}/{c.n_kv_heads})"
        assert c.intermediate_size % tp_world == 0
        self.n_heads = c.n_heads // tp_world
        self.n_kv_heads = c.n_kv_heads // tp_world
        self.inter = c.intermediate_size // tp_world
        self.q_size = self.n_heads * c.head_dim
        self.kv_size = self.n_kv_heads * c.head_dim
        self.scale = 1.0 / math.sqrt(c.head_dim)
        self.params: dict[str, torch.Tensor] = {}
        # per-request LoRA adapters (load_adapter): name -> stack index,
        # the source tensors per adapter, and the stacked device tensors
        # the batched kernels read (None until the first adapter loads)
        self.adapter_names: list[str] = []
        self._adapter_src: dict[str, dict] = {}
        self.lora: Optional[dict] = None
        self.lora_scale: Optional[torch.Tensor] = None
        self.lora_slices: dict[str, list] = {}
        self._w4_scratch: Optional[torch.Tensor] = None
        self._w4_slab: Optional[torch.Tensor] = None
        self._w4_tiled = True       # False inside forward_prefill
        self._init_weights(seed)
        if self.quant == "fp8":
            self._quantize_weights()
        elif self.quant == "int4":
            self._quantize_weights_int4()
        elif self.quant == "int4-awq":
            self._quantize_weights_awq()
        self.cos_sin = ops.build_cos_sin(c.max_position, c.head_dim,
                                         c.rope_theta, device=self.device)

    # ------------------------------------------------------------ weights
    def _mk(self, name: str, shape: tuple, gen: torch.Generator,
            std: float = 0.02) -> None:
        t = torch.empty(shape, dtype=self.dtype, device=self.device)
        t.normal_(0.0, std, generator=gen)
        self.params[name] = t

    def _full(self, shape: tuple, gen: torch.Generator,
              std: float = 0.02) -> torch.Tensor:
        t = torch.empty(shape, dtype=self.dtype, device=self.device)
        t.normal_(0.0, std, generator=gen)
        return t

    def _init_weights(self, seed: int) -> None:
        """Every rank draws the FULL weight with the same seed and keeps
        its shard — so TP=N computes the same function as TP=1 (the
        gloo/CPU TP tests rely on this)."""
        c = self.config
        r, w = self.tp_rank, self.tp_world
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed + 1)
        self._mk("embed", (c.vocab_size, c.hidden_size), gen)
        std_o = 0.02 / math.sqrt(2 * c.n_layers)
        for i in range(c.n_layers):
            gen.manual_seed(seed * 1000003 + i * 1009)
            qkv = self._full((c.q_size + 2 * c.kv_size, c.hidden_size), gen)
            qf, kf, vf = torch.split(qkv, [c.q_size, c.kv_size, c.kv_size], dim=0)
            self.params[f"l{i}.qkv"] = torch.cat([
                qf[r * self.q_size:(r + 1) * self.q_size],
                kf[r * self.kv_size:(r + 1) * self.kv_size],
                vf[r * self.kv_size:(r + 1) * self.kv_size]], dim=0).contiguous()
            o = self._full((c.hidden_size, c.q_size), gen, std_o)
            self.params[f"l{i}.o"] = o[:, r * self.q_size:(r + 1) * self.q_size].contiguous()
            if c.num_experts:
                E, I = c.num_experts, c.moe_intermediate_size
                # a wider router than 0.02 so that random weights spread
                # the tokens over the experts with distinct logits
                self._mk(f"l{i}.router", (E, c.hidden_size), gen, 0.5)
                self._mk(f"l{i}.experts_gate_up", (E, 2 * I, c.hidden_size),
                         gen)
                self._mk(f"l{i}.experts_down", (E, c.hidden_size, I), gen,
                         std_o)
            else:
                gu = self._full((2 * c.intermediate_size, c.hidden_size), gen)
                gf, uf = torch.split(gu, [c.intermediate_size, c.intermediate_size], dim=0)
                self.params[f"l{i}.gate_up"] = torch.cat([
                    gf[r * self.inter:(r + 1) * self.inter],
                    uf[r * self.inter:(r + 1) * self.inter]], dim=0).contiguous()
                down = self._full((c.hidden_size, c.intermediate_size), gen, std_o)
                self.params[f"l{i}.down"] = down[:, r * self.inter:(r + 1) * self.inter].contiguous()
            self.params[f"l{i}.ln1"] = torch.ones(c.hidden_size, dtype=self.dtype,
                                                  device=self.device)
            self.params[f"l{i}.ln2"] = torch.ones_like(self.params[f"l{i}.ln1"])
            if c.qk_norm:      # [head_dim]: replicated, not sharded, under TP
                self.params[f"l{i}.q_norm"] = torch.ones(
                    c.head_dim, dtype=self.dtype, device=self.device)
                self.params[f"l{i}.k_norm"] = torch.ones_like(
                    self.params[f"l{i}.q_norm"])
        gen.manual_seed(seed + 2)
        self.params["final_ln"] = torch.ones(c.hidden_size, dtype=self.dtype,
                                             device=self.device)
        if c.tie_embeddings:
            self.params["lm_head"] = self.params["embed"]
        else:
            self._mk("lm_head", (c.vocab_size, c.hidden_size), gen)

    def _quantize_weights(self) -> None:
        """Quantize gate_up/down/lm_head to fp8-e4m3 with per-out-channel
        scales and FREE the bf16 originals (8B: ~5.5 GiB back).  Called
        after random init and again after a safetensors load."""
        from ..ops import ref as _ref
        names = [f"l{i}.{n}" for i in range(self.config.n_layers)
                 for n in ("gate_up", "down")] + ["lm_head"]
        for name in names:
            w = self.params.get(name)
            if w is None or w.dtype != self.dtype:
                continue
            q, sc = _ref.quantize_fp8_rowwise(w)
            self.params[name + ".q8"] = q.contiguous()
            self.params[name + ".s"] = sc.to(torch.float32).contiguous()
            if name == "lm_head" and w is self.params.get("embed"):
                pass              # tied: keep the bf16 embed for lookups
            del self.params[name]

    def _linear_fp8(self, x8: torch.Tensor, xs: torch.Tensor,
                    name: str) -> torch.Tensor:
        w8 = self.params[name + ".q8"]
        ws = self.params[name + ".s"]
        if x8.is_cuda:
            return torch._scaled_mm(x8, w8.t(), scale_a=xs.reshape(-1, 1),
                                    scale_b=ws.reshape(1, -1),
                                    out_dtype=torch.bfloat16)
        from ..ops import ref as _ref
        return _ref.scaled_mm_ref(x8, xs, w8, ws)

    _W4_FUSED_ROWS = 64         # ops.w4a16_linear takes 1..64 rows
    # up to these rows the down projection takes gu itself and applies
    # SwiGLU in its A fragments (ops.w4a16_silu_linear, bit-identical to
    # silu_mul + w4a16_linear).  0: it measured slower than that pair at
    # every M on the 8B down shape (profiles/w4a16_silu.md), so no step
    # routes to it
    _W4_SILU_ROWS = 0
    _W4_TILED_ROWS = 256        # ops.w4a16_tiled_linear takes 65..256
    # (N, K) whose tiled launch was measured slower than dequantize + GEMM
    # above these rows (profiles/w4a16_tiled.md): the 8B qkv from 160 rows
    _W4_TILED_ROWS_BY_SHAPE = {(6144, 4096): 128}

    def _w4_tiled_rows(self, N: int, K: int) -> int:
        if not self._w4_tiled:
            return self._W4_FUSED_ROWS
        return min(self._W4_TILED_ROWS,
                   self._W4_TILED_ROWS_BY_SHAPE.get((N, K), 256))

    # (N, K): (first row, last row) that run ops.w4a16_wide_linear, ahead
    # of the tiled op and of dequantize + GEMM: only the shapes and rows
    # where it measured not slower than the path it replaces
    # (profiles/w4a16_wide.md).  Any other shape keeps the routing above.
    _W4_WIDE_ROWS_BY_SHAPE = {(28672, 4096): (224, 256),
                              (4096, 14336): (224, 256)}

    def _w4_wide(self, rows: int, N: int, K: int) -> bool:
        first, last = self._W4_WIDE_ROWS_BY_SHAPE.get((N, K), (1, 0))
        return self._w4_tiled and first <= rows <= last

    def _w4_shapes(self) -> dict:
        """Per-rank (after TP sharding) [N, K] of the int4 projections."""
        c = self.config
        return {"qkv": (self.q_size + 2 * self.kv_size, c.hidden_size),
                "o": (c.hidden_size, self.q_size),
                "gate_up": (2 * self.inter, c.hidden_size),
                "down": (c.hidden_size, self.inter)}

    def _quantize_weights_int4(self) -> None:
        """Quantize this rank's qkv/o/gate_up/down shards to group-128
        int4 (round-to-nearest) and FREE the bf16 originals.  Called
        after random init and again after a safetensors load."""
        from ..ops import ref as _ref
        shapes = self._w4_shapes()
        for i in range(self.config.n_layers):
            for n, (N, K) in shapes.items():
                name = f"l{i}.{n}"
                w = self.params.get(name)
                if w is None:
                    continue
                assert tuple(w.shape) == (N, K), (name, tuple(w.shape), N, K)
                assert N % 64 == 0 and K % _ref.W4_GROUP == 0, (
                    f"{name}: int4 needs N % 64 == 0 and K % 128 == 0 per "
                    f"rank, got N={N} K={K}")
                q, s = _ref.quantize_w4(w)
                self.params[name + ".q4"] = _ref.w4_pack(q)
                self.params[name + ".s4"] = s
                del self.params[name]
        self._w4_alloc_shared()

    def _quantize_weights_awq(self) -> None:
        """Random-initialised weights under quant="int4-awq": asymmetric
        group-128 round-to-nearest into the packed / meta pair a loaded
        AWQ checkpoint gives, bf16 originals freed."""
        from ..ops import ref as _ref
        for i in range(self.config.n_layers):
            for n in self._w4_shapes():
                name = f"l{i}.{n}"
                u, z, s = _ref.quantize_w4_zp(self.params.pop(name))
                self.params[name + ".q4"] = _ref.w4_pack(u.to(torch.int8) - 8)
                self.params[name + ".m4"] = _ref.w4_zp_meta(z, s)
        self._w4_alloc_shared()

    def _w4_alloc_shared(self) -> None:
        shapes = self._w4_shapes()
        if self.device.type == "cuda" and self._w4_scratch is None:
            # one dequant buffer for the largest projection and one
            # split-K slab for the widest launch, shared by all layers
            # (the stream orders their users): allocated here, once,
            # before any graph capture
            self._w4_scratch = torch.empty(
                max(N * K for N, K in shapes.values()),
                dtype=torch.bfloat16, device=self.device)
            def slab_rows(N, K):           # slices * rows, per launch form
                wide = self._W4_WIDE_ROWS_BY_SHAPE.get((N, K))
                return max(
                    ops.w4a16_plan(N, K)[0] * self._W4_FUSED_ROWS,
                    ops.w4a16_tiled_plan(N, K)[0] * self._W4_TILED_ROWS,
                    ops.w4a16_wide_plan(N, K)[0] * wide[1] if wide else 0)
            self._w4_slab = torch.empty(
                max(slab_rows(N, K) * N for N, K in shapes.values()),
                dtype=torch.float32, device=self.device)

    def _linear_w4(self, x: torch.Tensor, name: str) -> torch.Tensor:
        q4 = self.params[name + ".q4"]
        if self.quant == "int4-awq":
            m4 = self.params[name + ".m4"]
            if not x.is_cuda:
                return ops.w4a16_zp_linear(x, q4, m4)  # the reference
            if x.shape[0] <= self._W4_FUSED_ROWS:
                return ops.w4a16_zp_linear(x, q4, m4, ws=self._w4_slab)
            N, K = m4.shape[0], x.shape[1]
            if self._w4_wide(x.shape[0], N, K):
                return ops.w4a16_zp_wide_linear(x, q4, m4, ws=self._w4_slab)
            if x.shape[0] <= self._w4_tiled_rows(N, K):
                return ops.w4a16_zp_tiled_linear(x, q4, m4, ws=self._w4_slab)
            w = ops.w4_zp_dequant(
                q4, m4, out=self._w4_scratch[:N * K].view(N, K))
            return _linear(x, w)
        s4 = self.params[name + ".s4"]
        if not x.is_cuda:
            return ops.w4a16_linear(x, q4, s4)     # the reference
        if x.shape[0] <= self._W4_FUSED_ROWS:
            return ops.w4a16_linear(x, q4, s4, ws=self._w4_slab)
        N, K = s4.shape[0], x.shape[1]
        if self._w4_wide(x.shape[0], N, K):
            return ops.w4a16_wide_linear(x, q4, s4, ws=self._w4_slab)
        if x.shape[0] <= self._w4_tiled_rows(N, K):
            return ops.w4a16_tiled_linear(x, q4, s4, ws=self._w4_slab)
        w = ops.w4_dequant(q4, s4, out=self._w4_scratch[:N * K].view(N, K))
        return _linear(x, w)

    def _linear_w4_silu(self, gu: torch.Tensor, name: str) -> torch.Tensor:
        """``_linear_w4(ops.silu_mul(gu), name)`` in one launch, for the
        at most ``_W4_SILU_ROWS`` rows ``_layer_w4`` sends here."""
        q4 = self.params[name + ".q4"]
        if self.quant == "int4-awq":
            return ops.w4a16_zp_silu_linear(gu, q4, self.params[name + ".m4"],
                                            ws=self._w4_slab)
        return ops.w4a16_silu_linear(gu, q4, self.params[name + ".s4"],
                                     ws=self._w4_slab)

    def load_safetensors(self, path: str) -> int:
        """Load HF-Llama-named safetensors shards, TP-sharded at load
        (VERDICT r01 #3): each rank takes its column slice of q/k/v and
        gate/up and its row slice of o/down — the exact layout
        ``_init_weights`` produces, so TP=N computes the same function as
        TP=1 on the same checkpoint.  Returns the number of tensors
        consumed.  (The reference runs real models in every pool —
        /root/reference/src/demo_account_sharding.py:202-224.)"""
        import safetensors.torch as st
        c = self.config
        r = self.tp_rank
        loaded = 0
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no .safetensors files under {path}")
        raw: dict[str, torch.Tensor] = {}
        for f in files:
            raw.update(st.load_file(os.path.join(path, f)))
        is_awq = any(k.endswith(".qweight") for k in raw)
        if is_awq != (self.quant == "int4-awq"):
            raise ValueError(
                f"{path} holds {'AWQ int4' if is_awq else 'dense'} weights "
                f"but the model was built with quant={self.quant!r}: "
                + ("AWQ checkpoints load under quant='int4-awq' only"
                   if is_awq else "quant='int4-awq' loads AWQ checkpoints "
                   "only (nothing is quantized at load)"))
        self._check_qk_norm_keys(raw, path)
        self._check_moe_keys(raw, path)
        if is_awq:
            return self._load_awq(raw, path)

        def take(name, rows: Optional[int] = None, cols: Optional[int] = None):
            """Move to device taking only this rank's shard: ``rows`` =
            per-rank output rows (column-parallel), ``cols`` = per-rank
            input columns (row-parallel)."""
            nonlocal loaded
            t = raw[name]
            if rows is not None:
                t = t[r * rows:(r + 1) * rows]
            if cols is not None:
                t = t[:, r * cols:(r + 1) * cols]
            loaded += 1
            return t.to(self.dtype).to(self.device).contiguous()

        self.params["embed"] = take("model.embed_tokens.weight")
        for i in range(c.n_layers):
            p = f"model.layers.{i}."
            q = take(p + "self_attn.q_proj.weight", rows=self.q_size)
            k = take(p + "self_attn.k_proj.weight", rows=self.kv_size)
            v = take(p + "self_attn.v_proj.weight", rows=self.kv_size)
            self.params[f"l{i}.qkv"] = torch.cat([q, k, v], dim=0).contiguous()
            self.params[f"l{i}.o"] = take(p + "self_attn.o_proj.weight",
                                          cols=self.q_size)
            if c.num_experts:
                self.params[f"l{i}.router"] = take(p + "mlp.gate.weight")
                x = p + "mlp.experts."
                self.params[f"l{i}.experts_gate_up"] = torch.stack([
                    torch.cat([take(f"{x}{j}.gate_proj.weight"),
                               take(f"{x}{j}.up_proj.weight")], dim=0)
                    for j in range(c.num_experts)]).contiguous()
                self.params[f"l{i}.experts_down"] = torch.stack([
                    take(f"{x}{j}.down_proj.weight")
                    for j in range(c.num_experts)]).contiguous()
            else:
                g = take(p + "mlp.gate_proj.weight", rows=self.inter)
                u = take(p + "mlp.up_proj.weight", rows=self.inter)
                self.params[f"l{i}.gate_up"] = torch.cat([g, u], dim=0).contiguous()
                self.params[f"l{i}.down"] = take(p + "mlp.down_proj.weight",
                                                 cols=self.inter)
            self.params[f"l{i}.ln1"] = take(p + "input_layernorm.weight")
            self.params[f"l{i}.ln2"] = take(p + "post_attention_layernorm.weight")
            if c.qk_norm:
                self.params[f"l{i}.q_norm"] = take(p + "self_attn.q_norm.weight")
                self.params[f"l{i}.k_norm"] = take(p + "self_attn.k_norm.weight")
        self.params["final_ln"] = take("model.norm.weight")
        if "lm_head.weight" in raw:
            self.params["lm_head"] = take("lm_head.weight")
        else:
            self.params["lm_head"] = self.params["embed"]
        if self.quant == "fp8":
            self._quantize_weights()
        elif self.quant == "int4":
            self._quantize_weights_int4()
        return loaded

    def _check_qk_norm_keys(self, raw: dict, path: str) -> None:
        """The checkpoint holds ``self_attn.{q,k}_norm.weight`` for every
        layer exactly when the model has a q/k norm: a key the model would
        drop, or one it would miss, names itself here."""
        c = self.config
        want = [f"model.layers.{i}.self_attn.{n}_norm.weight"
                for i in range(c.n_layers) for n in "qk"]
        if c.qk_norm:
            for key in want:
                if key not in raw:
                    raise ValueError(
                        f"{path} has no {key}: {c.name} has a q/k norm "
                        f"(qk_norm=True) and the checkpoint does not")
                if tuple(raw[key].shape) != (c.head_dim,):
                    raise ValueError(
                        f"{path}: {key} has shape {tuple(raw[key].shape)}, "
                        f"the model [{c.head_dim}]")
            return
        for key in sorted(raw):
            if key.endswith(("self_attn.q_norm.weight",
                             "self_attn.k_norm.weight")):
                raise ValueError(
                    f"{path} holds {key} but {c.name} has no q/k norm "
                    f"(qk_norm=False): the weight would be dropped")

    def _check_moe_keys(self, raw: dict, path: str) -> None:
        """A Mixture-of-Experts model needs the router (``mlp.gate.weight``)
        and every expert's three projections, at the model's shapes, and no
        dense ``mlp.{gate,up,down}_proj``; a dense model the reverse.  The
        first key that is missing, misshapen or would be dropped names
        itself."""
        c = self.config
        E, I, H = c.num_experts, c.moe_intermediate_size, c.hidden_size
        if not E:
            for key in sorted(raw):
                if ".mlp.experts." in key or key.endswith(".mlp.gate.weight"):
                    raise ValueError(
                        f"{path} holds {key} but {c.name} has a dense MLP "
                        f"(num_experts=0): the weight would be dropped")
            return
        for i in range(c.n_layers):
            p = f"model.layers.{i}.mlp."
            for n in ("gate_proj", "up_proj", "down_proj"):
                if f"{p}{n}.weight" in raw:
                    raise ValueError(
                        f"{path} holds {p}{n}.weight but {c.name} is a "
                        f"Mixture-of-Experts model (num_experts={E}): the "
                        f"dense MLP weight would be dropped")
            want = {p + "gate.weight": (E, H)}
            for j in range(E):
                want[f"{p}experts.{j}.gate_proj.weight"] = (I, H)
                want[f"{p}experts.{j}.up_proj.weight"] = (I, H)
                want[f"{p}experts.{j}.down_proj.weight"] = (H, I)
            for key, shape in want.items():
                if key not in raw:
                    raise ValueError(
                        f"{path} has no {key}: {c.name} is a Mixture-of-"
                        f"Experts model (num_experts={E}) and the checkpoint "
                        f"does not hold it")
                if tuple(raw[key].shape) != shape:
                    raise ValueError(
                        f"{path}: {key} has shape {tuple(raw[key].shape)}, "
                        f"the model {list(shape)}")

    _AWQ_CONFIG = {"quant_method": "awq", "bits": 4, "group_size": 128,
                   "version": "gemm", "zero_point": True}

    @classmethod
    def _check_awq_config(cls, path: str) -> None:
        """``config.json``'s quantization_config, when there is one, must
        describe the one layout the repack kernel reads."""
        import json
        cfg_path = os.path.join(path, "config.json")
        if not os.path.exists(cfg_path):
            return
        with open(cfg_path) as f:
            qc = json.load(f).get("quantization_config")
        if qc is None:
            return
        for field, want in cls._AWQ_CONFIG.items():
            got = qc.get(field)
            if isinstance(want, str) and isinstance(got, str):
                got = got.lower()
            if got != want or type(got) is not type(want):
                raise ValueError(
                    f"{cfg_path}: quantization_config.{field} must be "
                    f"{want!r}, got {qc.get(field)!r}")

    def _load_awq(self, raw: dict, path: str) -> int:
        """An AutoAWQ Llama checkpoint (GEMM layout, 4 bits, group 128):
        every projection's qweight / qzeros / scales go to the device as
        they are and ``ops.awq_repack`` writes them into the fused
        packed / meta pair - q/k/v and gate/up at their column offsets.
        embed, norms and lm_head are cast to the model dtype."""
        from ..ops import ref as _ref
        self._check_awq_config(path)
        c = self.config
        loaded = 0

        def dense(name):
            nonlocal loaded
            loaded += 1
            return raw[name].to(self.dtype).to(self.device).contiguous()

        def fused(i, n, parts):
            nonlocal loaded
            N, K = self._w4_shapes()[n]
            packed = torch.empty(N * K // 8, dtype=torch.int32,
                                 device=self.device)
            meta = torch.empty((N, K // _ref.W4_GROUP), dtype=torch.int32,
                               device=self.device)
            col = 0
            for part in parts:
                base = f"model.layers.{i}.{part}."
                qw, qz, sc = (raw[base + t].to(self.device).contiguous()
                              for t in ("qweight", "qzeros", "scales"))
                if qw.shape[0] != K:
                    raise ValueError(f"{base}qweight has K={qw.shape[0]}, "
                                     f"the model {K}")
                ops.awq_repack(qw, qz, sc, packed, meta, col)
                col += sc.shape[1]
                loaded += 3
            if col != N:
                raise ValueError(f"layer {i} {n}: checkpoint has {col} "
                                 f"output columns, the model {N}")
            self.params.pop(f"l{i}.{n}", None)
            self.params[f"l{i}.{n}.q4"] = packed
            self.params[f"l{i}.{n}.m4"] = meta

        self.params["embed"] = dense("model.embed_tokens.weight")
        for i in range(c.n_layers):
            fused(i, "qkv", [f"self_attn.{x}_proj" for x in "qkv"])
            fused(i, "o", ["self_attn.o_proj"])
            fused(i, "gate_up", ["mlp.gate_proj", "mlp.up_proj"])
            fused(i, "down", ["mlp.down_proj"])
            p = f"model.layers.{i}."
            self.params[f"l{i}.ln1"] = dense(p + "input_layernorm.weight")
            self.params[f"l{i}.ln2"] = dense(
                p + "post_attention_layernorm.weight")
            if c.qk_norm:
                self.params[f"l{i}.q_norm"] = dense(
                    p + "self_attn.q_norm.weight")
                self.params[f"l{i}.k_norm"] = dense(
                    p + "self_attn.k_norm.weight")
        self.params["final_ln"] = dense("model.norm.weight")
        self.params["lm_head"] = dense("lm_head.weight") \
            if "lm_head.weight" in raw else self.params["embed"]
        self._w4_alloc_shared()
        return loaded

    def save_safetensors(self, path: str) -> None:
        if self.quant is not None:
            raise RuntimeError("cannot save a weight-quantized model "
                               "(bf16 originals were freed)")
        """Write the FULL (unsharded) weights in HF-Llama naming — the
        round-trip fixture for the TP-sharded-load tests.  TP=1 only."""
        import safetensors.torch as st
        assert self.tp_world == 1, "save from an unsharded model"
        c = self.config
        out: dict[str, torch.Tensor] = {}
        out["model.embed_tokens.weight"] = self.params["embed"]
        for i in range(c.n_layers):
            p = f"model.layers.{i}."
            qkv = self.params[f"l{i}.qkv"]
            q, k, v = torch.split(qkv, [c.q_size, c.kv_size, c.kv_size], dim=0)
            out[p + "self_attn.q_proj.weight"] = q
            out[p + "self_attn.k_proj.weight"] = k
            out[p + "self_attn.v_proj.weight"] = v
            out[p + "self_attn.o_proj.weight"] = self.params[f"l{i}.o"]
            if c.num_experts:
                I = c.moe_intermediate_size
                out[p + "mlp.gate.weight"] = self.params[f"l{i}.router"]
                for j in range(c.num_experts):
                    x = f"{p}mlp.experts.{j}."
                    gu = self.params[f"l{i}.experts_gate_up"][j]
                    out[x + "gate_proj.weight"] = gu[:I]
                    out[x + "up_proj.weight"] = gu[I:]
                    out[x + "down_proj.weight"] = \
                        self.params[f"l{i}.experts_down"][j]
            else:
                gu = self.params[f"l{i}.gate_up"]
                g, u = torch.split(gu, [c.intermediate_size, c.intermediate_size], dim=0)
                out[p + "mlp.gate_proj.weight"] = g
                out[p + "mlp.up_proj.weight"] = u
                out[p + "mlp.down_proj.weight"] = self.params[f"l{i}.down"]
            out[p + "input_layernorm.weight"] = self.params[f"l{i}.ln1"]
            out[p + "post_attention_layernorm.weight"] = self.params[f"l{i}.ln2"]
            if c.qk_norm:
                out[p + "self_attn.q_norm.weight"] = self.params[f"l{i}.q_norm"]
                out[p + "self_attn.k_norm.weight"] = self.params[f"l{i}.k_norm"]
        out["model.norm.weight"] = self.params["final_ln"]
        if self.params["lm_head"] is not self.params["embed"]:
            out["lm_head.weight"] = self.params["lm_head"]
        os.makedirs(path, exist_ok=True)
        st.save_file({k: v.contiguous().cpu() for k, v in out.items()},
                     os.path.join(path, "model.safetensors"))

    # ----------------------------------------------------------- adapters
    # HF/PEFT module -> (fused projection, slice within it)
    _LORA_MODULES = {"q_proj": ("qkv", 0), "k_proj": ("qkv", 1),
                     "v_proj": ("qkv", 2), "o_proj": ("o", 0),
                     "gate_proj": ("gate_up", 0), "up_proj": ("gate_up", 1),
                     "down_proj": ("down", 0)}
    LORA_MAX_RANK = 64

    def _lora_geometry(self) -> dict:
        """Fused projection -> (input width K, [slice widths])."""
        c = self.config
        return {"qkv": (c.hidden_size, [self.q_size, self.kv_size,
                                        self.kv_size]),
                "o": (self.q_size, [c.hidden_size]),
                "gate_up": (c.hidden_size, [self.inter, self.inter]),
                "down": (self.inter, [c.hidden_size])}

    @staticmethod
    def _peft_key(i: int, module: str, which: str) -> str:
        block = "mlp" if module in ("gate_proj", "up_proj", "down_proj") \
            else "self_attn"
        return (f"base_model.model.model.layers.{i}.{block}.{module}."
                f"lora_{which}.weight")

    def adapter_index(self, name: str) -> int:
        return self.adapter_names.index(name)

    def add_adapter(self, name: str, r: int, lora_alpha: float,
                    target_modules, weights: dict) -> None:
        """Register one LoRA adapter from PEFT-named tensors
        (``...layers.{i}.self_attn.q_proj.lora_A.weight`` [r, in] and
        ``lora_B.weight`` [out, r]) and rebuild the stacks.  q/k/v and
        gate/up fold into the fused qkv and gate_up projections as rank
        slices; a module the adapter does not target gets zero B.  A name
        already loaded is replaced in place (same stack index)."""
        if self.tp_world > 1:
            raise RuntimeError("LoRA adapters are not supported with "
                               "tensor_parallel > 1")
        if self.quant is not None:
            raise RuntimeError("LoRA adapters are not supported on a "
                               "weight-quantized model")
        if self.config.num_experts:
            raise RuntimeError("LoRA adapters are not supported on a "
                               "Mixture-of-Experts model")
        r = int(r)
        if not 1 <= r <= self.LORA_MAX_RANK:
            raise ValueError(f"adapter {name!r}: r must be in 1.."
                             f"{self.LORA_MAX_RANK}, got {r}")
        targets = sorted(target_modules)
        unknown = [m for m in targets if m not in self._LORA_MODULES]
        if unknown:
            raise ValueError(f"adapter {name!r}: unsupported "
                             f"target_modules {unknown}")
        geo = self._lora_geometry()
        tensors: dict[str, torch.Tensor] = {}
        for i in range(self.config.n_layers):
            for m in targets:
                proj, s = self._LORA_MODULES[m]
                K, widths = geo[proj]
                for which, shape in (("A", (r, K)), ("B", (widths[s], r))):
                    key = self._peft_key(i, m, which)
                    if key not in weights:
                        raise KeyError(f"adapter {name!r}: missing {key}")
                    t = weights[key]
                    if tuple(t.shape) != shape:
                        raise ValueError(
                            f"adapter {name!r}: {key} has shape "
                            f"{tuple(t.shape)}, expected {shape}")
                    tensors[key] = t.to(self.dtype).contiguous().cpu()
        self._adapter_src[name] = {"r": r, "lora_alpha": float(lora_alpha),
                                   "target_modules": targets,
                                   "tensors": tensors}
        if name not in self.adapter_names:
            self.adapter_names.append(name)
        self._rebuild_adapter_stack()

    def _rebuild_adapter_stack(self) -> None:
        """Stack every loaded adapter per fused projection: A
        [n, n_slices * r_max, K] and B [n, O, r_max], zero-padded to the
        largest rank loaded.  Runs on load, never on a hot path."""
        n = len(self.adapter_names)
        srcs = [self._adapter_src[a] for a in self.adapter_names]
        r_max = max(s["r"] for s in srcs)
        geo = self._lora_geometry()
        lora: dict[str, tuple] = {}
        for proj, (K, widths) in geo.items():
            ends, lo = [], 0
            for w in widths:
                lo += w
                ends.append(lo)
            self.lora_slices[proj] = ends
        for i in range(self.config.n_layers):
            for proj, (K, widths) in geo.items():
                A = torch.zeros((n, len(widths) * r_max, K), dtype=self.dtype)
                B = torch.zeros((n, sum(widths), r_max), dtype=self.dtype)
                for ai, src in enumerate(srcs):
                    r = src["r"]
                    for m in src["target_modules"]:
                        mproj, s = self._LORA_MODULES[m]
                        if mproj != proj:
                            continue
                        lo = sum(widths[:s])
                        A[ai, s * r_max:s * r_max + r] = \
                            src["tensors"][self._peft_key(i, m, "A")]
                        B[ai, lo:lo + widths[s], :r] = \
                            src["tensors"][self._peft_key(i, m, "B")]
                lora[f"l{i}.{proj}"] = (A.to(self.device), B.to(self.device))
        self.lora = lora
        self.lora_scale = torch.tensor(
            [s["lora_alpha"] / s["r"] for s in srcs], dtype=torch.float32,
            device=self.device)

    def load_adapter(self, name: str, path: str) -> None:
        """Load a PEFT LoRA directory: ``adapter_config.json`` (r,
        lora_alpha, target_modules) + ``adapter_model.safetensors``."""
        import json
        import safetensors.torch as st
        with open(os.path.join(path, "adapter_config.json")) as f:
            cfg = json.load(f)
        weights = st.load_file(os.path.join(path,
                                            "adapter_model.safetensors"))
        self.add_adapter(name, cfg["r"], cfg["lora_alpha"],
                         cfg["target_modules"], weights)

    def save_adapter(self, name: str, path: str) -> str:
        """Write a loaded adapter back as a PEFT directory — the
        round-trip fixture for the adapter tests.  Returns ``path``."""
        import json
        import safetensors.torch as st
        src = self._adapter_src[name]
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "adapter_config.json"), "w") as f:
            json.dump({"peft_type": "LORA", "r": src["r"],
                       "lora_alpha": src["lora_alpha"],
                       "target_modules": src["target_modules"]}, f)
        st.save_file(dict(src["tensors"]),
                     os.path.join(path, "adapter_model.safetensors"))
        return path

    def _lora_add_(self, key: str, proj: str, x: torch.Tensor,
                   out: torch.Tensor, adapter_idx: torch.Tensor) -> torch.Tensor:
        """out += the per-row low-rank update of projection ``key``, next
        to (after) its base GEMM: one shrink and one expand launch."""
        if self.lora is None:
            raise RuntimeError("adapter_idx given but no adapter is loaded")
        A, B = self.lora[key]
        y = ops.lora_shrink(x.contiguous(), A, adapter_idx)
        return ops.lora_expand_add_(out, y, B, self.lora_scale,
                                    self.lora_slices[proj], adapter_idx)

    def param_bytes(self) -> int:
        seen = set()
        total = 0
        for t in self.params.values():
            if id(t) not in seen:
                seen.add(id(t))
                total += t.numel() * t.element_size()
        return total

    # ------------------------------------------------------------ compute
    def _all_reduce(self, x: torch.Tensor) -> torch.Tensor:
        if self.tp_world > 1:
            import torch.distributed as dist
            dist.all_reduce(x, group=self.tp_group)
        return x

    def _layer(self, i: int, x: torch.Tensor, residual: Optional[torch.Tensor],
               positions: torch.Tensor, kv_cache, slot_mapping: torch.Tensor,
               attn_fn, adapter_idx: Optional[torch.Tensor] = None
               ) -> tuple[torch.Tensor, torch.Tensor]:
        """``adapter_idx`` ([T] int32, -1 = none): per-row LoRA adapter;
        each of the four projections is then followed by a shrink and an
        expand on its output (o and down: before the all-reduce and the
        residual).  None executes nothing new."""
        p = self.params
        c = self.config
        if adapter_idx is not None:
            return self._layer_lora(i, x, residual, kv_cache, attn_fn,
                                    adapter_idx)
        if residual is None:
            residual = x.clone()
            h = ops.rmsnorm(x, p[f"l{i}.ln1"], c.rms_eps)
        else:
            h = ops.rmsnorm_residual_(x, residual, p[f"l{i}.ln1"], c.rms_eps)
        if self.quant in ("int4", "int4-awq"):
            return self._layer_w4(i, h, residual, kv_cache, attn_fn)
        qkv = _linear(h, p[f"l{i}.qkv"])
        k_cache, v_cache = kv_cache.layer(i)
        # rope + cache append happen inside attn_fn (the decode path fuses
        # them into the attention kernel itself)
        attn_out = attn_fn(i, qkv, k_cache, v_cache)   # [T, q_size]
        h = self._all_reduce(_linear(attn_out, p[f"l{i}.o"]))
        if self.quant == "fp8":
            h2q, h2s = ops.rmsnorm_residual_fp8(h, residual, p[f"l{i}.ln2"],
                                                c.rms_eps)
            gu = self._linear_fp8(h2q, h2s, f"l{i}.gate_up")
            dq, ds = ops.silu_mul_fp8(gu)
            mlp = self._all_reduce(self._linear_fp8(dq, ds, f"l{i}.down"))
            return mlp, residual
        h2 = ops.rmsnorm_residual_(h, residual, p[f"l{i}.ln2"], c.rms_eps)
        if c.num_experts:
            ids, w = ops.moe_route(_linear(h2, p[f"l{i}.router"]),
                                   c.experts_per_token, c.norm_topk_prob)
            mlp = ops.moe_mlp(h2, ids, w, p[f"l{i}.experts_gate_up"],
                              p[f"l{i}.experts_down"])
            return mlp, residual
        gu = _linear(h2, p[f"l{i}.gate_up"])
        mlp = self._all_reduce(_linear(ops.silu_mul(gu), p[f"l{i}.down"]))
        return mlp, residual

    def _layer_w4(self, i: int, h: torch.Tensor, residual: torch.Tensor,
                  kv_cache, attn_fn) -> tuple[torch.Tensor, torch.Tensor]:
        """``_layer`` after the first norm with the four projections on
        int4 weights."""
        p = self.params
        c = self.config
        qkv = self._linear_w4(h, f"l{i}.qkv")
        k_cache, v_cache = kv_cache.layer(i)
        attn_out = attn_fn(i, qkv, k_cache, v_cache)   # [T, q_size]
        h = self._all_reduce(self._linear_w4(attn_out, f"l{i}.o"))
        h2 = ops.rmsnorm_residual_(h, residual, p[f"l{i}.ln2"], c.rms_eps)
        gu = self._linear_w4(h2, f"l{i}.gate_up")
        if gu.is_cuda and gu.shape[0] <= self._W4_SILU_ROWS:
            down = self._linear_w4_silu(gu, f"l{i}.down")
        else:
            down = self._linear_w4(ops.silu_mul(gu), f"l{i}.down")
        mlp = self._all_reduce(down)
        return mlp, residual

    def _layer_lora(self, i: int, x: torch.Tensor,
                    residual: Optional[torch.Tensor], kv_cache, attn_fn,
                    adapter_idx: torch.Tensor
                    ) -> tuple[torch.Tensor, torch.Tensor]:
        """``_layer`` with the low-rank update after every projection
        (bf16 weights only: adapters do not load on a quantized model)."""
        p = self.params
        c = self.config
        if residual is None:
            residual = x.clone()
            h = ops.rmsnorm(x, p[f"l{i}.ln1"], c.rms_eps)
        else:
            h = ops.rmsnorm_residual_(x, residual, p[f"l{i}.ln1"], c.rms_eps)
        qkv = self._lora_add_(f"l{i}.qkv", "qkv", h,
                              _linear(h, p[f"l{i}.qkv"]), adapter_idx)
        k_cache, v_cache = kv_cache.layer(i)
        attn_out = attn_fn(i, qkv, k_cache, v_cache)   # [T, q_size]
        h = self._all_reduce(self._lora_add_(
            f"l{i}.o", "o", attn_out, _linear(attn_out, p[f"l{i}.o"]),
            adapter_idx))
        h2 = ops.rmsnorm_residual_(h, residual, p[f"l{i}.ln2"], c.rms_eps)
        gu = self._lora_add_(f"l{i}.gate_up", "gate_up", h2,
                             _linear(h2, p[f"l{i}.gate_up"]), adapter_idx)
        act = ops.silu_mul(gu)
        mlp = self._all_reduce(self._lora_add_(
            f"l{i}.down", "down", act, _linear(act, p[f"l{i}.down"]),
            adapter_idx))
        return mlp, residual

    def _rope_kv_append(self, i: int, qkv: torch.Tensor,
                        positions: torch.Tensor, k_cache: torch.Tensor,
                        v_cache: torch.Tensor,
                        slot_mapping: torch.Tensor) -> None:
        """RoPE + cache append on layer i's raw qkv rows, after the q/k norm
        where the model has one (one kernel either way)."""
        if self.config.qk_norm:
            ops.qk_norm_rope_kv_append_qkv_(
                qkv, self.params[f"l{i}.q_norm"], self.params[f"l{i}.k_norm"],
                self.config.rms_eps, positions, self.cos_sin, k_cache,
                v_cache, slot_mapping, self.n_heads)
        else:
            ops.rope_kv_append_qkv_(qkv, positions, self.cos_sin, k_cache,
                                    v_cache, slot_mapping, self.n_heads)

    def forward_prefill(self, input_ids: torch.Tensor, positions: torch.Tensor,
                        kv_cache, slot_mapping: torch.Tensor,
                        cu_seqlens: torch.Tensor,
                        adapter_idx: Optional[torch.Tensor] = None
                        ) -> torch.Tensor:
        """Returns logits for the LAST token of each sequence:
        [n_seqs, vocab]."""
        def attn(i, qkv, k_cache, v_cache):
            self._rope_kv_append(i, qkv, positions, k_cache, v_cache,
                                 slot_mapping)
            return ops.prefill_attn_qkv(qkv, cu_seqlens, self.scale,
                                        self.n_heads, self.n_kv_heads,
                                        self.config.head_dim)
        # int4: a whole-prompt prefill keeps dequantize + GEMM above 64 rows
        self._w4_tiled = False
        try:
            return self._forward(input_ids, positions, kv_cache,
                                 slot_mapping, attn,
                                 last_idx=cu_seqlens[1:].long() - 1,
                                 adapter_idx=adapter_idx)
        finally:
            self._w4_tiled = True

    def forward_mixed(self, input_ids: torch.Tensor, positions: torch.Tensor,
                      kv_cache, slot_mapping: torch.Tensor, n_decode: int,
                      block_tables_dec, seq_lens_dec,
                      chunk_row0, chunk_pos0, chunk_nrows, chunk_btrow,
                      block_tables_pre, sample_idx,
                      adapter_idx: Optional[torch.Tensor] = None
                      ) -> torch.Tensor:
        """Mixed batch: rows [0, n_decode) are decode tokens, the rest
        are prefill-chunk tokens attending over the paged cache
        (chunked prefill).  Returns logits for ``sample_idx`` rows."""
        def attn(i, qkv, k_cache, v_cache):
            self._rope_kv_append(i, qkv, positions, k_cache, v_cache,
                                 slot_mapping)
            out = ops.prefill_paged_attn(
                qkv, k_cache, v_cache, chunk_row0, chunk_pos0, chunk_nrows,
                chunk_btrow, block_tables_pre, self.scale, self.n_heads)
            if n_decode:
                out_d = ops.decode_attn_qkv(
                    qkv[:n_decode], k_cache, v_cache, block_tables_dec,
                    seq_lens_dec, self.scale, self.n_heads)
                out[:n_decode] = out_d
            return out
        return self._forward(input_ids, positions, kv_cache, slot_mapping,
                             attn, last_idx=sample_idx,
                             adapter_idx=adapter_idx)

    def forward_decode(self, input_ids: torch.Tensor, positions: torch.Tensor,
                       kv_cache, slot_mapping: torch.Tensor,
                       block_tables: torch.Tensor,
                       seq_lens: torch.Tensor,
                       adapter_idx: Optional[torch.Tensor] = None,
                       shared_plan: Optional[tuple] = None
                       ) -> torch.Tensor:
        """One token per sequence; returns [batch, vocab] logits.  With a
        ``shared_plan`` (ops.decode_attn_shared_qkv) rows that share
        leading KV blocks read them once per group; the plan's workspace
        serves every layer."""
        def attn(i, qkv, k_cache, v_cache):
            if shared_plan is not None:
                self._rope_kv_append(i, qkv, positions, k_cache, v_cache,
                                     slot_mapping)
                return ops.decode_attn_shared_qkv(
                    qkv, k_cache, v_cache, block_tables, seq_lens,
                    shared_plan, self.scale, self.n_heads)
            if self.config.qk_norm:
                return ops.decode_attn_qknorm_rope_qkv(
                    qkv, self.params[f"l{i}.q_norm"],
                    self.params[f"l{i}.k_norm"], self.config.rms_eps,
                    positions, self.cos_sin, k_cache, v_cache, slot_mapping,
                    block_tables, seq_lens, self.scale, self.n_heads)
            return ops.decode_attn_rope_qkv(
                qkv, positions, self.cos_sin, k_cache, v_cache, slot_mapping,
                block_tables, seq_lens, self.scale, self.n_heads)
        return self._forward(input_ids, positions, kv_cache, slot_mapping,
                             attn, last_idx=None, adapter_idx=adapter_idx)

    def _forward(self, input_ids, positions, kv_cache, slot_mapping, attn_fn,
                 last_idx, adapter_idx=None) -> torch.Tensor:
        p = self.params
        x = F.embedding(input_ids.long(), p["embed"])
        residual = None
        for i in range(self.config.n_layers):
            x, residual = self._layer(i, x, residual, positions, kv_cache,
                                      slot_mapping, attn_fn, adapter_idx)
        if self.quant == "fp8":
            h8, hs = ops.rmsnorm_residual_fp8(x, residual, p["final_ln"],
                                              self.config.rms_eps)
            if last_idx is not None:
                h8 = h8[last_idx]
                hs = hs[last_idx]
            return self._linear_fp8(h8, hs, "lm_head")
        h = ops.rmsnorm_residual_(x, residual, p["final_ln"],
                                  self.config.rms_eps)
        if last_idx is not None:
            h = h[last_idx]
        return _linear(h, p["lm_head"])   # bf16 logits feed ops.sample
