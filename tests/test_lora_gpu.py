"""The batched LoRA HIP kernels against the torch reference — exact-integer
bit equality over the shape grid, poisoned surroundings, 1-ulp agreement
on random bf16 data, determinism — and per-request adapters through the
bf16 engine on the device, beside the captured decode graph."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config

from lora_cases import (O_VALUES, RANK_CASES, SHAPES,
                        bf16_ulp_distance, integer_case, random_adapter,
                        random_case, ref_out, run_idx_of)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
GUARD = 1031            # odd: out starts on no 4-, 8- or 16-byte boundary


def run_device(case, guard=0):
    """shrink + expand on the device; ``out`` lives inside a NaN-filled
    buffer with ``guard`` elements on both sides.  Returns (y, out, the
    whole buffer) on the CPU."""
    T, O = case["out"].shape
    buf = torch.full((2 * guard + T * O,), float("nan"), dtype=BF16,
                     device=DEV)
    out = buf[guard:guard + T * O].view(T, O)
    out.copy_(case["out"])
    idx = case["idx"].to(DEV)
    y = ops.lora_shrink(case["x"].to(DEV), case["A"].to(DEV), idx)
    got = ops.lora_expand_add_(out, y, case["B"].to(DEV),
                               case["scale"].to(DEV), case["slices"], idx)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return y.cpu(), out.cpu(), buf.cpu()


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("r_max,n_slices", RANK_CASES)
def test_exact_integers_bit_equal_and_poison_intact(r_max, n_slices):
    changed = 0
    for T, K, O in SHAPES:
        case = integer_case(T, K, O, r_max, n_slices)
        y_ref, out_ref = ref_out(case)
        y, out, buf = run_device(case, guard=GUARD)
        tag = (T, K, O)
        used = case["idx"] >= 0
        assert torch.equal(y[used], y_ref[used]), tag
        assert torch.equal(bits(out), bits(out_ref)), tag
        # rows without an adapter: bit-unchanged
        assert torch.equal(bits(out[~used]), bits(case["out"][~used])), tag
        changed += int((bits(out[used]) != bits(case["out"][used])).sum())
        # guard regions on both sides still all-NaN
        assert bool(buf[:GUARD].isnan().all()), tag
        assert bool(buf[GUARD + T * O:].isnan().all()), tag
    assert changed > 0          # the adapter rows really were updated


@pytest.mark.parametrize("r_max,n_slices", RANK_CASES)
def test_random_bf16_within_one_ulp(r_max, n_slices):
    """Both sides round once from f32 sums that differ only in order: every
    element within 1 bf16 ulp, fewer than 1 % of them different at all
    (tests/test_lora_ref.py holds the reference's own shuffled order to
    the same allowance on this data)."""
    worst_frac = 0.0
    for T, K, O in SHAPES:
        case = random_case(T, K, O, r_max, n_slices)
        _, out_ref = ref_out(case)
        _, out, _ = run_device(case)
        d = bf16_ulp_distance(out, out_ref)
        frac = float((d != 0).float().mean())
        worst_frac = max(worst_frac, frac)
        assert int(d.max()) <= 1, (T, K, O, int(d.max()))
        assert frac < 0.01, (T, K, O, frac)
        used = case["idx"] >= 0
        assert torch.equal(bits(out[~used]), bits(case["out"][~used]))
    print(f"r_max={r_max} n_slices={n_slices}: worst mismatch fraction "
          f"{worst_frac:.2e}")


@pytest.mark.parametrize("r_max,n_slices", RANK_CASES)
def test_token_tiles_with_runs_of_one_adapter(r_max, n_slices):
    """From 512 rows up a workgroup covers 4 consecutive tokens and loads A
    / the B row once when they share an adapter.  515 rows in runs of 6
    per adapter hit shared, mixed and partly adapter-free tiles and a
    ragged last tile: still bit-equal to the reference on integers, and on
    random data bit-equal to the same rows run as a small (untiled) batch
    — the result of a row does not depend on its neighbours or on T."""
    T = 515
    for K in (8, 520, 4096):
        for O in O_VALUES:
            case = integer_case(T, K, O, r_max, n_slices)
            case["idx"] = run_idx_of(T)
            _, out_ref = ref_out(case)
            _, out, buf = run_device(case, guard=GUARD)
            assert torch.equal(bits(out), bits(out_ref)), (K, O)
            assert bool(buf[:GUARD].isnan().all())
            assert bool(buf[GUARD + T * O:].isnan().all())
    case = random_case(T, 520, 264, r_max, n_slices)
    case["idx"] = run_idx_of(T)
    _, out, _ = run_device(case)
    head = dict(case, x=case["x"][:60], out=case["out"][:60],
                idx=case["idx"][:60])
    _, out_head, _ = run_device(head)
    assert torch.equal(bits(out[:60]), bits(out_head))
    assert int(bf16_ulp_distance(out, ref_out(case)[1]).max()) <= 1
    # the rows of one prompt: every tile shares its adapter
    case["idx"] = torch.full((T,), 2, dtype=torch.int32)
    _, out, _ = run_device(case)
    assert int(bf16_ulp_distance(out, ref_out(case)[1]).max()) <= 1
    case = integer_case(T, 256, 264, r_max, n_slices)
    case["idx"] = torch.full((T,), 1, dtype=torch.int32)
    assert torch.equal(bits(run_device(case)[1]), bits(ref_out(case)[1]))


@pytest.mark.parametrize("shape", [(257, 4096, 6144, 64, 3),
                                   (65, 520, 264, 16, 2),
                                   (3, 8, 8, 1, 1)], ids=str)
def test_two_calls_are_bit_identical(shape):
    case = random_case(*shape)
    y1, out1, _ = run_device(case)
    y2, out2, _ = run_device(case)
    used = case["idx"] >= 0
    assert torch.equal(y1[used].view(torch.int32), y2[used].view(torch.int32))
    assert torch.equal(bits(out1), bits(out2))


def test_unaligned_and_odd_widths_take_the_scalar_arm():
    """K and r_max that are no multiple of 8, O odd, and x/A/B views that
    start off a 16-byte boundary."""
    T, K, O, r_max = 5, 77, 131, 5
    g = torch.Generator().manual_seed(11)

    def ints(shape):
        return torch.randint(-2, 3, shape, generator=g).to(BF16)
    case = dict(x=ints((T, K)), A=ints((2, 2 * r_max, K)),
                B=ints((2, O, r_max)), out=ints((T, O)),
                scale=torch.tensor([0.5, 2.0]), slices=[64, O],
                idx=torch.tensor([1, 0, -1, 1, 0], dtype=torch.int32))
    y_ref, out_ref = ref_out(case)
    y, out, _ = run_device(case, guard=GUARD)
    assert torch.equal(bits(out), bits(out_ref))
    # 16-byte-wide shapes behind an odd element offset
    case = integer_case(3, 256, 264, 8, 2)
    _, out_ref = ref_out(case)
    idx = case["idx"].to(DEV)

    def shifted(t):
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:] = t.flatten()
        return flat[1:].view(t.shape)
    out = shifted(case["out"])
    y = ops.lora_shrink(shifted(case["x"]), shifted(case["A"]), idx)
    ops.lora_expand_add_(out, y, shifted(case["B"]), case["scale"].to(DEV),
                         case["slices"], idx)
    assert torch.equal(bits(out.cpu()), bits(out_ref))


def test_wrapper_rejects_bad_arguments():
    case = integer_case(3, 256, 264, 8, 2)
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v)
         for k, v in case.items()}
    y = ops.lora_shrink(d["x"], d["A"], d["idx"])
    with pytest.raises(RuntimeError):
        ops.lora_shrink(d["x"].float(), d["A"], d["idx"])
    with pytest.raises(RuntimeError):
        ops.lora_shrink(d["x"], d["A"], d["idx"].long())
    with pytest.raises(RuntimeError):
        ops.lora_shrink(d["x"], d["A"], d["idx"][:2])
    with pytest.raises(RuntimeError):
        ops.lora_shrink(d["x"], d["A"][:, :, :128].contiguous(), d["idx"])
    args = (d["B"], d["scale"])
    with pytest.raises(RuntimeError):       # last boundary != O
        ops.lora_expand_add_(d["out"], y, *args, [130, 200], d["idx"])
    with pytest.raises(RuntimeError):       # not ascending
        ops.lora_expand_add_(d["out"], y, *args, [264, 130], d["idx"])
    with pytest.raises(RuntimeError):       # y width != n_slices * r_max
        ops.lora_expand_add_(d["out"], y, *args, [264], d["idx"])
    with pytest.raises(RuntimeError):       # r_max > 64
        ops.lora_expand_add_(
            d["out"], torch.zeros((3, 72), device=DEV),
            torch.zeros((3, 264, 72), dtype=BF16, device=DEV), d["scale"],
            [264], d["idx"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ engine
def make_engine(adapters=True, graphs=False, **kw):
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=3)
    if adapters:
        model.add_adapter("zero", *random_adapter(model, 8, seed=1,
                                                  zero_b=True))
        model.add_adapter("x", *random_adapter(model, 8, seed=2, std=0.3))
        model.add_adapter("y", *random_adapter(model, 16, seed=3, std=0.3,
                                               targets=("q_proj", "v_proj",
                                                        "down_proj")))
    kv = PagedKVCache.for_model(cfg, 256, device=DEV)
    kw.setdefault("enable_prefix_caching", False)
    kw.setdefault("max_batch_size", 8)
    engine = LLMEngine(model, kv, **kw)
    if graphs:
        from resilient_llm_amd.engine.graph import install_graph_runner
        install_graph_runner(engine)
    return engine


def drain(engine, max_steps=1000):
    outs = {}
    for _ in range(max_steps):
        if not engine.has_work():
            break
        for o in engine.step():
            outs.setdefault(o.req_id, []).append(o.token_id)
    assert not engine.has_work()
    return outs


def prompt_of(n, k=7):
    return [5 + (k * i) % 90 for i in range(n)]


GREEDY = SamplingParams(max_tokens=16, temperature=0.0, stop_on_eos=False)


def test_zero_b_adapter_gives_the_base_tokens_in_the_same_batch():
    def run(adapter):
        e = make_engine()
        e.add_request("a", prompt_of(37), GREEDY, adapter=adapter)
        e.add_request("b", prompt_of(21, 11), GREEDY, adapter="x")
        e.add_request("c", prompt_of(9, 3), GREEDY)
        return drain(e)
    with_zero, without = run("zero"), run(None)
    assert with_zero == without
    assert len(with_zero["a"]) == 16


def test_adapters_change_greedy_tokens():
    e = make_engine()
    e.add_request("x", prompt_of(37), GREEDY, adapter="x")
    e.add_request("y", prompt_of(37), GREEDY, adapter="y")
    e.add_request("n", prompt_of(37), GREEDY)
    outs = drain(e)
    assert outs["x"] != outs["n"] and outs["y"] != outs["n"]
    assert outs["x"] != outs["y"]
    assert e.kv.free_blocks == e.kv.num_blocks


def test_adapter_batches_run_eager_beside_the_graph_path():
    """Adapter-free batches before and after a mixed adapter batch replay
    the captured graph; the adapter batch's 16 decode steps do not; the
    adapter-free tokens equal an engine's that never loaded an adapter."""
    e = make_engine(graphs=True)
    calls = []
    real_step = e.graph_runner.step

    def spy():
        calls.append(e.step_count)
        return real_step()
    e.graph_runner.step = spy

    def phase(reqs):
        n0 = len(calls)
        for rid, prompt, adapter in reqs:
            e.add_request(rid, prompt, GREEDY, adapter=adapter)
        return drain(e), len(calls) - n0

    free_before, n_before = phase([("p0", prompt_of(37), None),
                                   ("p1", prompt_of(21, 11), None)])
    mixed, n_mixed = phase([("mx", prompt_of(37), "x"),
                            ("my", prompt_of(21, 11), "y"),
                            ("mn", prompt_of(9, 3), None)])
    free_after, n_after = phase([("q0", prompt_of(37), None),
                                 ("q1", prompt_of(21, 11), None)])
    assert n_before >= 14 and n_after >= 14      # 15 decode steps each
    assert n_mixed == 0
    assert e.stats["decode_steps"] >= 45
    assert all(len(v) == 16 for v in mixed.values())

    plain = make_engine(adapters=False, graphs=True)
    for rid, prompt in (("p0", prompt_of(37)), ("p1", prompt_of(21, 11))):
        plain.add_request(rid, prompt, GREEDY)
    want = drain(plain)
    assert free_before == want
    assert {"p0": free_after["q0"], "p1": free_after["q1"]} == want
    assert mixed["mx"] != free_before["p0"]
