"""The tiled int4-weight HIP kernel (1 <= M <= 256), symmetric and
zero-point form, on the device: exact-integer and needle bit equality with
NaN-poisoned ``out`` / slab / x surroundings, forced K-slicing against the
register ring, the random-data bound of the existing contract, row
independence across M, the wrapper's checks, ``_linear_w4``'s routing by
rows and an int4 engine at decode batch 80."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

import awq_cases
import w4a16_cases
from w4a16_cases import BF16, GROUP, describe, forced_slices, n_edge_sweeps
from test_w4a16_gpu import bits, drain

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
# (M, N, K, splitk).  A second wave with one live row, one group; one wave
# and an odd group count; 2, 3, 4 waves; the down-proj K; a wide N; then
# forced slicing: 3, 3, 3, 2 groups per slice under four waves (register
# ring of 4 groups) and 5, 5 under two (ring of 2, LDS double buffer)
SHAPES = [(65, 64, 128, 0), (64, 64, 384, 0), (128, 128, 512, 0),
          (129, 192, 1024, 0), (200, 64, 2048, 0), (256, 256, 512, 0),
          (256, 64, 14336, 0), (100, 6144, 256, 0), (256, 64, 1408, 4),
          (100, 128, 1280, 2)]
FORMS = {"sym": (w4a16_cases, "w4a16_tiled_linear"),
         "zp": (awq_cases, "w4a16_zp_tiled_linear")}
ids = lambda s: "x".join(map(str, s))        # noqa: E731
forms = pytest.mark.parametrize("form", list(FORMS))


def tiled_slices(N, K, splitk=0):
    """The documented slicing: whole groups, ceil(256 / panels) slices but
    at least 4 groups in a slice, ceil(groups / slices) groups per slice,
    no empty slice; ``forced_slices`` under a caller's ``splitk``."""
    groups = K // GROUP
    sk = min(max(1, -(-256 // (N // 64))), max(1, groups // 4))
    sl = forced_slices(K, splitk or sk)
    assert ops.w4a16_tiled_plan(N, K, splitk) == (len(sl), sl[0][1] - sl[0][0])
    return sl


def run(form, case, splitk=0, x=None, **kw):
    sm = case.meta if form == "zp" else case.s
    return getattr(ops, FORMS[form][1])(
        case.x.to(DEV) if x is None else x, case.packed.to(DEV), sm.to(DEV),
        splitk, **kw)


@forms
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_integers_bit_equal_in_poisoned_surroundings(form, shape):
    """``out`` and x are the first M rows of NaN-filled buffers one row
    longer, the slab is NaN-filled: the result is bit-equal to the oracle
    (so finite), the row after ``out`` is untouched, the row after x is
    never read."""
    M, N, K, splitk = shape
    slices = tiled_slices(N, K, splitk)
    if splitk:
        assert all((k1 - k0) // GROUP % 4 for k0, k1 in slices)
    case = FORMS[form][0].exact_case(M, N, K, slices=slices)
    buf = torch.full((M + 1, N), NAN, dtype=BF16, device=DEV)
    xbuf = torch.full((M + 1, K), NAN, dtype=BF16, device=DEV)
    xbuf[:M] = case.x.to(DEV)
    ws = torch.full((len(slices) * M * N,), NAN, device=DEV)
    got = run(form, case, splitk, x=xbuf[:M], out=buf[:M],
              ws=ws if len(slices) > 1 else None)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got.cpu(), case.expected), describe(got.cpu(), case)
    assert bool(buf[M].isnan().all())
    # the op's own allocations give the same bits
    assert torch.equal(bits(run(form, case, splitk)), bits(got))


@forms
@pytest.mark.parametrize("M", [64, 128, 192, 256])
def test_needles_bit_equal_per_wave_count(form, M):
    """One sweep holds 0, 7, 8, 31, 32, 127, 128, K-1 and both sides of the
    slice boundary; every wave count."""
    N, K = 128, 1024
    slices = tiled_slices(N, K)
    assert len(slices) == 2 and n_edge_sweeps(M, K, slices) == 1
    mod = FORMS[form][0]
    case = mod.needle_case(M, N, K, mod.needle_weights(N, K), slices=slices)
    out = run(form, case).cpu()
    assert torch.equal(out, case.expected), describe(out, case)


@forms
@pytest.mark.parametrize("shape", [(96, 256, 1024), (256, 64, 4096)], ids=ids)
def test_random_bf16_within_the_existing_bound(form, shape):
    """|got - y64| <= 2^-8 |y64| + 2^-19 S, the bound of w4a16_linear."""
    mod = FORMS[form][0]
    case = mod.random_case(*shape)
    y, allowed, _ = mod.random_bound(case)
    err = (run(form, case).cpu().double() - y).abs()
    print(f"{form} tiled random {shape}: max err/allowed "
          f"{float((err / allowed).max()):.3f}")
    assert bool((err <= allowed).all()), float((err / allowed).max())


@forms
def test_rows_do_not_depend_on_M(form):
    case = FORMS[form][0].random_case(256, 128, 1024)
    x = case.x.to(DEV)
    full = run(form, case)
    for m in (64, 65):
        part = run(form, case, x=x[:m])
        assert torch.equal(bits(full[:m]), bits(part)), m


def test_argument_checks():
    case = w4a16_cases.exact_case(3, 64, 1024)
    packed, s = case.packed.to(DEV), case.s.to(DEV)

    def x(M, K=1024):
        return torch.zeros(M, K, dtype=BF16, device=DEV)
    ops.w4a16_tiled_linear(x(256), packed, s)
    with pytest.raises(RuntimeError, match="1 <= M <= 256"):
        ops.w4a16_tiled_linear(x(257), packed, s)
    with pytest.raises(RuntimeError):                       # K % 128
        ops.w4a16_tiled_linear(x(3, 1088), packed, s)
    with pytest.raises(RuntimeError, match="N % 64"):
        ops.w4a16_tiled_linear(x(3), packed[:32 * 1024 // 8],
                               s[:32].contiguous())
    assert len(tiled_slices(64, 1024)) > 1
    with pytest.raises(RuntimeError, match="slices\\*M\\*N"):
        ops.w4a16_tiled_linear(x(3), packed, s, ws=torch.empty(8, device=DEV))


@pytest.mark.parametrize("quant", ["int4", "int4-awq"])
def test_linear_w4_routes_by_rows(quant):
    """100 rows: the tiled op's result, the dequant scratch untouched; 300
    rows: the scratch is written."""
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=3, quant=quant)
    op, sfx = ((ops.w4a16_zp_tiled_linear, ".m4") if quant == "int4-awq"
               else (ops.w4a16_tiled_linear, ".s4"))
    x = torch.randn(300, cfg.hidden_size,
                    generator=torch.Generator().manual_seed(1)).to(BF16).to(DEV)
    model._w4_scratch.fill_(7.0)
    got = model._linear_w4(x[:100], "l0.qkv")
    want = op(x[:100], model.params["l0.qkv.q4"], model.params["l0.qkv" + sfx])
    assert torch.equal(bits(got), bits(want))
    assert bool((model._w4_scratch == 7.0).all())
    model._linear_w4(x, "l0.qkv")
    assert not bool((model._w4_scratch == 7.0).all())


def test_int4_engine_at_batch_80_against_the_reference_op(monkeypatch):
    """80 greedy requests under max_batch_size=96 complete and free every
    block; their decode steps run the tiled op with 80 rows (the
    whole-prompt prefill before them keeps dequantize + GEMM).  The same
    engine with the tiled op replaced by the reference op
    ``ref.w4a16_linear`` gives the same prefill token and the same first
    decoded token for every request; later tokens may part on near-ties
    (the agreement is printed)."""
    rows, real = [], ops.w4a16_tiled_linear
    spy = lambda x, *a, **kw: (rows.append(x.shape[0]),          # noqa: E731
                               real(x, *a, **kw))[1]
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=5, quant="int4")
    outs = []
    for op in (spy, lambda x, packed, s, **kw: ref.w4a16_linear(x, packed, s)):
        monkeypatch.setattr(ops, "w4a16_tiled_linear", op)
        kv = PagedKVCache.for_model(cfg, 128, device=DEV)
        eng = LLMEngine(model, kv, max_batch_size=96)
        for i in range(80):
            eng.add_request(f"r{i}", [(7 * i + 3 * t) % 500 + 5
                                      for t in range(3)],
                            SamplingParams(max_tokens=4))
        outs.append(drain(eng))
        assert kv.free_blocks == kv.num_blocks
    got, want = outs
    assert rows and set(rows) == {80}
    assert len(got) == 80 and all(len(v) == 4 for v in got.values())
    same = sum(a == b for r in got for a, b in zip(got[r], want[r]))
    print(f"int4 batch 80: {same} of {4 * 80} tokens equal the reference's")
    assert all(got[r][:2] == want[r][:2] for r in got)
