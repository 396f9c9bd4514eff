"""Copy-on-fork on the GPU: the kv_copy_blocks_ HIP kernel against the
torch reference as raw bytes (every dtype, repeated sources, offsets past
32 bits), and n > 1 groups through the bf16 / fp8 engine, eager and
graphed."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn


def random_bits(shape, dtype, seed):
    """A tensor whose every BIT is random (NaN patterns included): the
    copy is compared as bytes, never as numbers."""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator(device="cpu").manual_seed(seed)
    raw = torch.randint(0, 256, (n * torch.empty((), dtype=dtype)
                                 .element_size(),), dtype=torch.uint8,
                        generator=g)
    return raw.view(dtype).view(shape).to(DEV)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


CASES = [
    (torch.bfloat16, (2, 8, 1, 16, 128)),
    (torch.bfloat16, (3, 9, 2, 16, 64)),
    (FP8, (2, 8, 1, 16, 64)),              # 1 KiB chunk, the smallest
    (torch.float32, (2, 8, 1, 16, 128)),
]
PAIRS = [
    ([2], [5]),                            # P = 1
    ([1, 1, 1, 4, 6], [0, 3, 7, 2, 5]),    # P = 5, one source three times
    ([], []),                              # P = 0: launches nothing
]


@pytest.mark.parametrize("dtype,shape", CASES,
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("src,dst", PAIRS, ids=["P1", "P5", "P0"])
def test_kernel_matches_reference_bytes(dtype, shape, src, dst):
    k = random_bits(shape, dtype, 1)
    v = random_bits(shape, dtype, 2)
    k0, v0 = k.clone(), v.clone()
    k_ref, v_ref = k.clone(), v.clone()
    ref.kv_copy_blocks_(k_ref, v_ref, i32(src), i32(dst))
    ops.kv_copy_blocks_(k, v, i32(src), i32(dst))
    torch.cuda.synchronize()
    for got, want, snap in ((k, k_ref, k0), (v, v_ref, v0)):
        got, want, snap = (t.view(torch.uint8) for t in (got, want, snap))
        assert torch.equal(got, want)
        for s, d in zip(src, dst):
            assert torch.equal(got[:, d], snap[:, s])
        untouched = [b for b in range(shape[1]) if b not in dst]
        assert torch.equal(got[:, untouched], snap[:, untouched])


def test_wrapper_rejects_bad_arguments():
    k = torch.zeros((2, 4, 1, 16, 64), dtype=torch.bfloat16, device=DEV)
    v = torch.zeros_like(k)
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(k, v, i32([0, 1]), i32([2]))
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(k, v, i32([0]).long(), i32([2]).long())
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(k, v.float(), i32([0]), i32([2]))
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(k.transpose(0, 1), v.transpose(0, 1),
                            i32([0]), i32([1]))
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(k, v, torch.tensor([0], dtype=torch.int32),
                            i32([1]))
    # a 12-byte chunk is not a multiple of 16
    odd = torch.zeros((1, 4, 1, 2, 3), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.kv_copy_blocks_(odd, odd.clone(), i32([0]), i32([1]))


def test_offsets_past_32_bits():
    """~4.6 GB per tensor: layer 1's blocks lie past byte 2^32, and
    block 69999 past it even within layer 0's neighbourhood arithmetic."""
    shape = (2, 70000, 8, 16, 128)
    k = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    v = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    assert k.numel() * 2 > 2 ** 32
    watched = [2, 3, 4, 5, 6, 69997, 69998, 69999]
    blk = shape[2:]
    for t, seed in ((k, 10), (v, 20)):
        for layer in range(2):
            for b in watched:
                t[layer, b] = random_bits(blk, torch.bfloat16,
                                          seed + 100 * layer + b % 97)
    snap = {(name, layer, b): t[layer, b].clone()
            for name, t in (("k", k), ("v", v))
            for layer in range(2) for b in watched}
    ops.kv_copy_blocks_(k, v, i32([69998, 3]), i32([69999, 5]))
    torch.cuda.synchronize()
    for name, t in (("k", k), ("v", v)):
        for layer in range(2):
            def same(b, as_b):
                return torch.equal(t[layer, b].view(torch.int16),
                                   snap[(name, layer, as_b)].view(torch.int16))
            assert same(69999, 69998) and same(5, 3)
            assert not torch.equal(snap[(name, layer, 5)].view(torch.int16),
                                   snap[(name, layer, 3)].view(torch.int16))
            for b in (2, 3, 4, 6, 69997, 69998):
                assert same(b, b), (name, layer, b)
    del k, v, snap
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ engine
def make_engine(model_name, num_blocks=64, seed=3, kv_dtype=torch.bfloat16,
                fill=None, **kw):
    cfg = get_config(model_name)
    model = LlamaForCausalLM(cfg, device=DEV, dtype=torch.bfloat16, seed=seed)
    kv = PagedKVCache.for_model(cfg, num_blocks, device=DEV,
                                kv_dtype=kv_dtype)
    if fill is not None:
        kv.k.copy_(torch.full(kv.k.shape, fill, device=DEV))
        kv.v.copy_(torch.full(kv.v.shape, fill, device=DEV))
    kw.setdefault("enable_prefix_caching", False)
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


def prompt_of(n):
    return [5 + (7 * i) % 90 for i in range(n)]


RIDS = [f"g.c{i}" for i in range(4)]


def sampled_group(engine, plen=37, max_tokens=12):
    engine.add_request_group(
        RIDS, prompt_of(plen),
        [SamplingParams(max_tokens=max_tokens, temperature=0.8, seed=100 + i)
         for i in range(4)])


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
@pytest.mark.parametrize("plen", [17, 37])
def test_greedy_group_gives_identical_lists(model_name, plen):
    e = make_engine(model_name)
    greedy = SamplingParams(max_tokens=12, temperature=0.0)
    e.add_request_group(RIDS, prompt_of(plen), [greedy] * 4)
    outs = drain(e)
    assert e.stats["forks"] == 3
    assert len(outs[RIDS[0]]) >= 1
    assert all(outs[r] == outs[RIDS[0]] for r in RIDS)
    assert e.kv.free_blocks == e.kv.num_blocks


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_sampled_group_deterministic_and_poison_proof(model_name):
    """Two fresh engines agree, and so does one whose cache held a finite
    poison (96.0) in every slot: a child that read a slot the fork did
    not copy would differ."""
    e1 = make_engine(model_name)
    sampled_group(e1)
    first = drain(e1)
    assert set(first) == set(RIDS) and e1.stats["forks"] == 3
    assert len({tuple(v) for v in first.values()}) > 1
    e2 = make_engine(model_name)
    sampled_group(e2)
    assert drain(e2) == first
    e3 = make_engine(model_name, fill=96.0)
    assert float(e3.kv.k.float().min()) == 96.0
    sampled_group(e3)
    assert drain(e3) == first


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_graph_runner_group_matches_eager(model_name):
    from resilient_llm_amd.engine.graph import install_graph_runner
    eager = make_engine(model_name, num_blocks=256, max_batch_size=8, seed=9)
    sampled_group(eager)
    eager_out = drain(eager)
    graphed = make_engine(model_name, num_blocks=256, max_batch_size=8,
                          seed=9)
    install_graph_runner(graphed)
    sampled_group(graphed)
    assert drain(graphed) == eager_out
    assert graphed.stats["forks"] == 3


@pytest.mark.parametrize("model_name", ["tiny", "tiny-128"])
def test_fp8_cache_greedy_group(model_name):
    e = make_engine(model_name, kv_dtype=FP8)
    assert e.kv.k.dtype == FP8
    e.add_request_group(RIDS, prompt_of(37),
                        [SamplingParams(max_tokens=12, temperature=0.0)] * 4)
    outs = drain(e)
    assert e.stats["forks"] == 3
    assert all(outs[r] == outs[RIDS[0]] for r in RIDS)
    assert e.kv.free_blocks == e.kv.num_blocks
