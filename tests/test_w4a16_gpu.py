"""The int4-weight HIP kernels on the device: exact-integer and needle
bit equality over the shape grid, poisoned surroundings and workspace,
row independence across M, determinism, the random-data bound against
the float64 oracle, ``w4_dequant`` bit equality, and ``quant="int4"``
through the engine beside the captured decode graph."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

from w4a16_cases import (BF16, DEQUANT_SHAPES, RANDOM_SHAPES, RING_SHAPES,
                         SHAPES, dequant_case, describe, exact_case,
                         forced_slices, n_edge_sweeps, needle_case,
                         needle_weights, plan_slices, random_bound,
                         random_case)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1031            # odd: out starts on no 4-, 8- or 16-byte boundary


def bits(t):
    return t.contiguous().view(torch.int16)


def run(case, **kw):
    return ops.w4a16_linear(case.x.to(DEV), case.packed.to(DEV),
                            case.s.to(DEV), **kw).cpu()


def run_poisoned(case, splitk=0):
    """The op with ``out`` inside a NaN-filled bf16 buffer and its split-K
    slab inside a NaN-filled f32 buffer, ``GUARD`` elements on each side
    of both.  Returns (out, out buffer, slab buffer, slab elements)."""
    M, K = case.x.shape
    N = case.s.shape[0]
    n_ws = len(case.slices) * M * N if len(case.slices) > 1 else 0
    buf = torch.full((2 * GUARD + M * N,), float("nan"), dtype=BF16,
                     device=DEV)
    # 4 * (GUARD + 1) bytes in: the slab itself stays 16-byte aligned
    wbuf = torch.full((2 * (GUARD + 1) + n_ws,), float("nan"),
                      dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + M * N].view(M, N)
    ws = wbuf[GUARD + 1:GUARD + 1 + n_ws] if n_ws else None
    got = ops.w4a16_linear(case.x.to(DEV), case.packed.to(DEV),
                           case.s.to(DEV), splitk, out=out, ws=ws)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu(), wbuf.cpu(), n_ws


def test_plan_matches_the_documented_slicing():
    for _, N, K in SHAPES + RANDOM_SHAPES + [(1, 4096, 4096),
                                             (1, 28672, 4096),
                                             (1, 4096, 14336)]:
        sl = plan_slices(N, K)
        sk, per = ops.w4a16_plan(N, K)
        assert (sk, per) == (len(sl), sl[0][1] - sl[0][0]), (N, K, sl)
    # more than one slice is really exercised by the grid
    assert any(len(plan_slices(N, K)) > 1 for _, N, K in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integers_bit_equal_and_poison_intact(shape):
    M, N, K = shape
    case = exact_case(M, N, K)
    out, buf, wbuf, n_ws = run_poisoned(case)
    assert torch.equal(out, case.expected), describe(out, case)
    assert bool(buf[:GUARD].isnan().all())
    assert bool(buf[GUARD + M * N:].isnan().all())
    # the slab: guards untouched; every slab element was written (a slab
    # that is summed but not written would have put NaN into out)
    assert bool(wbuf[:GUARD + 1].isnan().all())
    assert bool(wbuf[GUARD + 1 + n_ws:].isnan().all())
    assert not bool(wbuf[GUARD + 1:GUARD + 1 + n_ws].isnan().any())
    # the op's own allocation gives the same bits
    assert torch.equal(bits(run(case)), bits(out))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_needles_bit_equal(shape):
    """out[m, n] == +-s[n, g(k_m)] * q[n, k_m] for needles at 0, 7, 8, 31,
    32, 127, 128, K-1 and both sides of every K-slice boundary."""
    M, N, K = shape
    weights = needle_weights(N, K)
    q, s, packed = weights
    packed_d, s_d = packed.to(DEV), s.to(DEV)
    slices = plan_slices(N, K)
    for sweep in range(n_edge_sweeps(M, K, slices)):
        case = needle_case(M, N, K, weights, sweep)
        out = ops.w4a16_linear(case.x.to(DEV), packed_d, s_d).cpu()
        assert torch.equal(out, case.expected), describe(out, case)


@pytest.mark.parametrize("shape", RING_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_ring_rounds_and_tail_bit_equal(shape):
    """The M <= 16 kernel's weight ring (4 groups) through more than one
    steady round and through a tail after a round, by a caller-chosen
    ``splitk``: exact integers with poisoned surroundings, and needles on
    both sides of every slice boundary."""
    M, N, K, splitk = shape
    slices = forced_slices(K, splitk)
    sk, per = ops.w4a16_plan(N, K, splitk)
    assert (sk, per) == (len(slices), slices[0][1] - slices[0][0])
    assert per // 128 > 4                   # more than one ring of groups
    case = exact_case(M, N, K, slices=slices)
    out, buf, wbuf, n_ws = run_poisoned(case, splitk=splitk)
    assert torch.equal(out, case.expected), describe(out, case)
    assert bool(buf[:GUARD].isnan().all())
    assert bool(buf[GUARD + M * N:].isnan().all())
    assert bool(wbuf[:GUARD + 1].isnan().all())
    assert bool(wbuf[GUARD + 1 + n_ws:].isnan().all())
    weights = needle_weights(N, K)
    packed_d, s_d = weights[2].to(DEV), weights[1].to(DEV)
    for sweep in range(n_edge_sweeps(M, K, slices)):
        case = needle_case(M, N, K, weights, sweep, slices=slices)
        out = ops.w4a16_linear(case.x.to(DEV), packed_d, s_d, splitk).cpu()
        assert torch.equal(out, case.expected), describe(out, case)


@pytest.mark.parametrize("N,K", [(256, 1024), (64, 14336)])
def test_rows_independent_of_M_and_deterministic(N, K):
    case = random_case(64, N, K)
    x = case.x.to(DEV)
    packed, s = case.packed.to(DEV), case.s.to(DEV)
    full = ops.w4a16_linear(x, packed, s)
    again = ops.w4a16_linear(x, packed, s)
    assert torch.equal(bits(full), bits(again))
    one = ops.w4a16_linear(x[:1].contiguous(), packed, s)
    assert torch.equal(bits(full[:1]), bits(one))
    m17 = ops.w4a16_linear(x[:17].contiguous(), packed, s)
    assert torch.equal(bits(full[:17]), bits(m17))
    assert torch.equal(bits(ops.w4a16_linear(x[:17].contiguous(), packed, s)),
                       bits(m17))
    # a row does not see its neighbours: other rows replaced by huge values
    x2 = torch.full_like(x, 3.0e38)
    x2[5] = x[5]
    assert torch.equal(bits(ops.w4a16_linear(x2, packed, s)[5]),
                       bits(full[5]))


@pytest.mark.parametrize("shape", RANDOM_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_random_bf16_within_the_bound(shape):
    """|got - y64| <= 2^-8 |y64| + 2^-19 S: one bf16 rounding (2x margin
    over half an ulp) plus f32 accumulation of the offset-binary form."""
    case = random_case(*shape)
    got = run(case).double()
    y, allowed, S = random_bound(case)
    err = (got - y).abs()
    # what one correct rounding cannot explain (half a bf16 ulp of y's
    # binade), in units of S: a lower bound of the f32 accumulation error
    half_ulp = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(1e-300)))
                          - 8)
    acc = ((err - half_ulp).clamp_min(0) / S).max()
    print(f"w4a16 random {shape}: max err/allowed "
          f"{float((err / allowed).max()):.3f}, max (err - half ulp)/S "
          f"{float(acc):.3e}")
    assert bool((err <= allowed).all()), float((err / allowed).max())


@pytest.mark.parametrize("shape", DEQUANT_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_w4_dequant_bit_equal_and_poison_intact(shape):
    N, K = shape
    packed, s, expected = dequant_case(N, K)
    buf = torch.full((2 * GUARD + N * K,), float("nan"), dtype=BF16,
                     device=DEV)
    out = buf[GUARD:GUARD + N * K].view(N, K)
    got = ops.w4_dequant(packed.to(DEV), s.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(expected))
    assert torch.equal(bits(out.cpu()), bits(ref.w4_dequant(packed, s)))
    host = buf.cpu()
    assert bool(host[:GUARD].isnan().all())
    assert bool(host[GUARD + N * K:].isnan().all())
    # an aligned, op-allocated out takes the vector-store path
    assert torch.equal(bits(ops.w4_dequant(packed.to(DEV), s.to(DEV)).cpu()),
                       bits(expected))


def test_argument_checks():
    case = exact_case(3, 64, 256)
    x, packed, s = case.x.to(DEV), case.packed.to(DEV), case.s.to(DEV)
    with pytest.raises(RuntimeError, match="1 <= M <= 64"):
        ops.w4a16_linear(torch.zeros(65, 256, dtype=BF16, device=DEV),
                         packed, s)
    with pytest.raises(RuntimeError, match="1 <= M <= 64"):
        ops.w4a16_linear(torch.zeros(0, 256, dtype=BF16, device=DEV),
                         packed, s)
    with pytest.raises(RuntimeError):                       # K mismatch
        ops.w4a16_linear(torch.zeros(3, 384, dtype=BF16, device=DEV),
                         packed, s)
    with pytest.raises(RuntimeError):                       # K % 128
        ops.w4a16_linear(torch.zeros(3, 192, dtype=BF16, device=DEV),
                         packed, s)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.w4a16_linear(x.float(), packed, s)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.w4a16_linear(x, packed, s.float())
    with pytest.raises(RuntimeError, match="int32"):
        ops.w4a16_linear(x, packed.long(), s)
    with pytest.raises(RuntimeError, match="N\\*K/8"):
        ops.w4a16_linear(x, packed[:-4], s)
    with pytest.raises(RuntimeError, match="N % 64"):
        ops.w4a16_linear(x, packed[:32 * 256 // 8], s[:32].contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.w4a16_linear(x.t().contiguous().t(), packed, s)
    with pytest.raises(RuntimeError):
        ops.w4_dequant(packed, s, out=torch.empty(64, 128, dtype=BF16,
                                                  device=DEV))
    with pytest.raises(RuntimeError):                       # slab too small
        big = exact_case(3, 64, 1024)
        assert len(big.slices) > 1
        ops.w4a16_linear(big.x.to(DEV), big.packed.to(DEV), big.s.to(DEV),
                         ws=torch.empty(8, device=DEV))


# ------------------------------------------------------------------ engine
def test_int4_on_the_gpu_needs_bf16():
    with pytest.raises(ValueError, match="bfloat16"):
        LlamaForCausalLM(get_config("tiny"), device=DEV,
                         dtype=torch.float32, quant="int4")


def make_engine(model_name, num_blocks=256, seed=5, **kw):
    cfg = get_config(model_name)
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=seed,
                             quant="int4")
    kv = PagedKVCache.for_model(cfg, num_blocks, device=DEV)
    return LLMEngine(model, kv, **kw)


def drain(engine, max_steps=1000):
    outs = {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o.token_id)
    assert not engine.has_work()
    return outs


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_int4_engine_batch_and_graph_matches_eager(model_name, monkeypatch):
    """A 3-request batch completes; one 70-token prompt crosses the
    dequant path (more than 64 rows) in prefill and the fused kernel in
    decode; the captured decode graph gives the eager tokens."""
    from resilient_llm_amd.engine.graph import install_graph_runner
    prompts = {"a": list(range(4, 74)), "b": list(range(9, 50)),
               "c": list(range(30, 37))}
    assert len(prompts["a"]) == 70

    calls = {"dequant": [], "fused": []}
    real_dequant, real_fused = ops.w4_dequant, ops.w4a16_linear

    def spy_dequant(packed, s, out=None):
        calls["dequant"].append(tuple(s.shape))
        return real_dequant(packed, s, out=out)

    def spy_fused(x, *a, **kw):
        calls["fused"].append(x.shape[0])
        return real_fused(x, *a, **kw)
    monkeypatch.setattr(ops, "w4_dequant", spy_dequant)
    monkeypatch.setattr(ops, "w4a16_linear", spy_fused)

    eager = make_engine(model_name, max_batch_size=8)
    assert eager.model._w4_scratch is not None
    for rid, p in prompts.items():
        eager.add_request(rid, p, SamplingParams(max_tokens=10))
    eager_out = drain(eager)
    assert all(len(v) == 10 for v in eager_out.values())
    # prefill really took the dequant path (more than 64 rows) for all four
    # projections, decode the fused kernel with a few rows
    cfg = eager.model.config
    assert {n for n, _ in calls["dequant"]} >= {
        cfg.q_size + 2 * cfg.kv_size, cfg.hidden_size,
        2 * cfg.intermediate_size}
    assert len(calls["dequant"]) % (4 * cfg.n_layers) == 0
    assert calls["fused"] and max(calls["fused"]) <= 64
    assert 3 in calls["fused"]

    graphed = make_engine(model_name, max_batch_size=8)
    install_graph_runner(graphed)
    for rid, p in prompts.items():
        graphed.add_request(rid, p, SamplingParams(max_tokens=10))
    assert drain(graphed) == eager_out


def _cpu_twin(gpu_model, cfg, quant):
    """CPU fp32 model holding the GPU model's exact weights (packed int4
    and bf16 scales stay as they are)."""
    twin = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=0,
                            quant=quant)
    for k, v in gpu_model.params.items():
        v = v.detach().cpu()
        twin.params[k] = v if k.endswith((".q4", ".s4")) else v.float()
    twin.cos_sin = gpu_model.cos_sin.cpu()
    return twin


def _logits_pair(model, cfg, device):
    """(prefill logits of one 40-token prompt, logits of one decode step
    of a batch of 3 after their prefills), float32 on the CPU."""
    f32 = model.dtype == torch.float32

    def kv_cache(nb):
        kv = PagedKVCache.for_model(cfg, nb, device=device)
        if f32:
            kv.k, kv.v = kv.k.float(), kv.v.float()
        return kv

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=device)
    bs = 16
    kv = kv_cache(8)
    ids = list(range(11, 51))
    pre = model.forward_prefill(i32(ids), i32(list(range(40))), kv,
                                i32(list(range(40))), i32([0, 40]))
    # three sequences of 20, 33 and 47 tokens, 4 blocks each
    lens = [20, 33, 47]
    kv = kv_cache(12)
    toks, pos, slots, cu = [], [], [], [0]
    for b, n in enumerate(lens):
        toks += [(7 * b + 3 * t) % cfg.vocab_size for t in range(n)]
        pos += list(range(n))
        slots += [b * 4 * bs + t for t in range(n)]
        cu.append(cu[-1] + n)
    model.forward_prefill(i32(toks), i32(pos), kv, i32(slots), i32(cu))
    bt = i32([[b * 4 + j for j in range(4)] for b in range(3)])
    dec = model.forward_decode(i32([5, 6, 7]), i32(lens), kv,
                               i32([b * 4 * bs + n
                                    for b, n in enumerate(lens)]),
                               bt, i32([n + 1 for n in lens]))
    return pre.float().cpu(), dec.float().cpu()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_int4_logits_against_cpu_fp32_twin(model_name):
    """max|err| / max|logit| of the int4 GPU model against the CPU fp32
    model holding the same packed weights is at most 2x the same measure
    of the unquantized bf16 GPU model against ITS CPU fp32 twin (the
    existing path), for a 40-token prefill (dequant is not involved: 40
    rows take the fused kernel; the 100-token batch prefill before the
    decode step does take it) and for one decode step of a batch of 3.
    Corrupting one group's scale on the CPU side breaks the bound."""
    cfg = get_config(model_name)
    dense = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=6)
    base = [_rel(g, c) for g, c in zip(
        _logits_pair(dense, cfg, DEV),
        _logits_pair(_cpu_twin(dense, cfg, None), cfg, "cpu"))]
    quant = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=6,
                             quant="int4")
    twin = _cpu_twin(quant, cfg, "int4")
    got_gpu = _logits_pair(quant, cfg, DEV)
    got = [_rel(g, c) for g, c in zip(got_gpu, _logits_pair(twin, cfg,
                                                            "cpu"))]
    print(f"{model_name}: int4 prefill/decode rel err {got[0]:.4e} "
          f"{got[1]:.4e}; bf16 baseline {base[0]:.4e} {base[1]:.4e}")
    # one wrong scale (x2 on one group of one row block) on the CPU side
    s4 = twin.params["l0.qkv.s4"].clone()
    s4[:, 1] = s4[:, 1] * 2
    twin.params["l0.qkv.s4"] = s4
    broken = [_rel(g, c) for g, c in zip(got_gpu, _logits_pair(twin, cfg,
                                                               "cpu"))]
    print(f"{model_name}: with one scale group doubled {broken[0]:.4e} "
          f"{broken[1]:.4e}")
    for what, g, b, br in zip(("prefill", "decode"), got, base, broken):
        assert g <= 2 * b, (what, g, b)
        assert br > 2 * b, (what, br, b)
