"""Measurements behind profiles/lora.md, on one GPU, Llama-3-8B shapes:

A. per-layer LoRA time — the four (shrink, expand) launch pairs of one
   layer (qkv, o, gate_up, down) at batch 1 / 32 / 256, r = 16 / 64, every
   row on one adapter or the rows spread over 4 adapters (interleaved
   t % 4, or grouped in 4 contiguous runs); device events
   around 100 repetitions, the cases alternated over 5 rounds;
B. eager decode step (model.forward_decode, no graph) at the same batches
   with no adapter row (the path the parent commit runs: nothing new
   executes), every row on one adapter, rows spread over 4 adapters;
C. prefill of one 1024-token prompt with and without an adapter.

Usage: python scripts/bench_lora.py [--out result.json] [--small]
(--small: the tiny-128 model and few repetitions — a CPU-side rehearsal
of the script's own logic is possible with --device cpu).
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from resilient_llm_amd import ops  # noqa: E402
from resilient_llm_amd.engine import PagedKVCache  # noqa: E402
from resilient_llm_amd.models import LlamaForCausalLM, get_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the results here")
ap.add_argument("--small", action="store_true")
ap.add_argument("--device", default=None)
args = ap.parse_args()
OUT = args.out

if args.device is None:
    assert torch.cuda.is_available(), "bench_lora needs a GPU"
DEV = args.device or "cuda:0"
ON_GPU = DEV.startswith("cuda")
MODEL = "tiny-128" if args.small else "llama-3-8b"
BATCHES = (1, 4) if args.small else (1, 32, 256)
RANKS = (16, 64)
REPS, ROUNDS = (3, 2) if args.small else (100, 5)
N_ADAPTERS = 4
CTX = 128                     # tokens already cached per decoding sequence
res = {"device": torch.cuda.get_device_name(0) if ON_GPU else "cpu",
       "model": MODEL}


def flush():
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


def sync():
    if ON_GPU:
        torch.cuda.synchronize()


def time_it(fn, reps):
    """us per call: device events on the GPU, host clock on the CPU."""
    if not ON_GPU:
        t0 = time.monotonic()
        for _ in range(reps):
            fn()
        return (time.monotonic() - t0) * 1e6 / reps
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def alternate(cases: dict, reps=REPS, rounds=ROUNDS) -> dict:
    """Median / min / max us per call of each case, the cases alternated."""
    for fn in cases.values():                       # warm every shape
        for _ in range(3):
            fn()
    sync()
    got = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            got[k].append(time_it(fn, reps))
    return {k: {"median_us": statistics.median(v), "min_us": min(v),
                "max_us": max(v)} for k, v in got.items()}


cfg = get_config(MODEL)
dtype = torch.bfloat16
model = LlamaForCausalLM(cfg, device=DEV, dtype=dtype, seed=0)
geo = model._lora_geometry()


def install_random_stack(r: int) -> None:
    """N_ADAPTERS random rank-r adapters straight into the model's stacked
    tensors (the timings do not depend on the values; building 8B-sized
    PEFT dictionaries on the host would only add minutes)."""
    g = torch.Generator(device=DEV).manual_seed(r)
    lora = {}
    for proj, (K, widths) in geo.items():
        ends, lo = [], 0
        for w in widths:
            lo += w
            ends.append(lo)
        model.lora_slices[proj] = ends
    for i in range(cfg.n_layers):
        for proj, (K, widths) in geo.items():
            A = torch.randn((N_ADAPTERS, len(widths) * r, K), device=DEV,
                            generator=g) * K ** -0.5
            B = torch.randn((N_ADAPTERS, sum(widths), r), device=DEV,
                            generator=g) * 0.02
            lora[f"l{i}.{proj}"] = (A.to(dtype), B.to(dtype))
    model.lora = lora
    model.adapter_names = [f"a{i}" for i in range(N_ADAPTERS)]
    model.lora_scale = torch.full((N_ADAPTERS,), 2.0, device=DEV)


def idx_of(case: str, T: int):
    if case == "none":
        return None
    if case == "one":
        return torch.zeros(T, dtype=torch.int32, device=DEV)
    if case == "four_grouped":          # 4 contiguous runs of rows
        return (torch.arange(T, device=DEV) * N_ADAPTERS // T).to(torch.int32)
    return (torch.arange(T, device=DEV) % N_ADAPTERS).to(torch.int32)


# ------------------------------------------------- A: per-layer LoRA time
res["layer"] = {}
for r in RANKS:
    install_random_stack(r)
    for B_ in BATCHES:
        xs = {proj: torch.randn((B_, K), device=DEV).to(dtype)
              for proj, (K, _) in geo.items()}
        outs = {proj: torch.randn((B_, sum(w)), device=DEV).to(dtype)
                for proj, (_, w) in geo.items()}

        def layer(idx):
            for proj in geo:
                A, Bm = model.lora[f"l0.{proj}"]
                y = ops.lora_shrink(xs[proj], A, idx)
                ops.lora_expand_add_(outs[proj], y, Bm, model.lora_scale,
                                     model.lora_slices[proj], idx)
        cases = {c: (lambda i=idx_of(c, B_): layer(i))
                 for c in ("one", "four", "four_grouped")}
        res["layer"][f"r{r}_b{B_}"] = alternate(cases)
        print(f"layer r={r} batch={B_}:",
              json.dumps(res["layer"][f"r{r}_b{B_}"]), flush=True)
flush()


# ---------------------------------------------------- B: eager decode step
def decode_inputs(B_):
    bs = 16
    n_blk = CTX // bs + 1
    kv = PagedKVCache.for_model(cfg, B_ * n_blk, device=DEV)
    bt = torch.arange(B_ * n_blk, dtype=torch.int32,
                      device=DEV).view(B_, n_blk)
    ids = torch.randint(5, cfg.vocab_size, (B_,), dtype=torch.int32,
                        device=DEV)
    pos = torch.full((B_,), CTX, dtype=torch.int32, device=DEV)
    slots = bt[:, CTX // bs] * bs + CTX % bs
    return kv, ids, pos, slots.to(torch.int32), bt, pos + 1


res["decode_step"] = {}
for r in RANKS:
    install_random_stack(r)
    for B_ in BATCHES:
        kv, ids, pos, slots, bt, lens = decode_inputs(B_)

        def step(idx):
            kw = {} if idx is None else {"adapter_idx": idx}
            return model.forward_decode(ids, pos, kv, slots, bt, lens, **kw)
        cases = {c: (lambda i=idx_of(c, B_): step(i))
                 for c in ("none", "one", "four", "four_grouped")}
        key = f"r{r}_b{B_}"
        res["decode_step"][key] = alternate(cases, reps=max(3, REPS // 5))
        print(f"decode step r={r} batch={B_}:",
              json.dumps(res["decode_step"][key]), flush=True)
        del kv
flush()

# -------------------------------------------- C: prefill of 1024 tokens
T = 64 if args.small else 1024
res["prefill_1k"] = {}
for r in RANKS:
    install_random_stack(r)
    kv = PagedKVCache.for_model(cfg, T // 16 + 1, device=DEV)
    ids = torch.randint(5, cfg.vocab_size, (T,), dtype=torch.int32,
                        device=DEV)
    pos = torch.arange(T, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)

    def prefill(idx):
        kw = {} if idx is None else {"adapter_idx": idx}
        return model.forward_prefill(ids, pos, kv, pos, cu, **kw)
    cases = {c: (lambda i=idx_of(c, T): prefill(i)) for c in ("none", "one")}
    res["prefill_1k"][f"r{r}"] = alternate(cases, reps=max(2, REPS // 10))
    print(f"prefill {T} tokens r={r}:",
          json.dumps(res["prefill_1k"][f"r{r}"]), flush=True)
flush()
