"""The wide int4-weight HIP kernel (1 <= M <= 512, 128-column panels),
symmetric and zero-point form, on the device: exact-integer and needle bit
equality with NaN-poisoned ``out`` / slab / x surroundings at every
row-block edge, forced K-slicing, the random-data bound of the existing
contract, row independence across M, the wrapper's checks and
``_linear_w4``'s routing through ``_W4_WIDE_ROWS_BY_SHAPE``."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.models import LlamaForCausalLM, get_config

import awq_cases
import w4a16_cases
from w4a16_cases import BF16, GROUP, describe, forced_slices, n_edge_sweeps
from test_w4a16_gpu import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
FORMS = {"sym": (w4a16_cases, "w4a16_wide_linear"),
         "zp": (awq_cases, "w4a16_zp_wide_linear")}
forms = pytest.mark.parametrize("form", list(FORMS))
# (N, K, splitk): one panel and two; one group, two groups in two slices
# (the slice boundary), 3 + 2 groups (uneven slices, both LDS buffers)
NK = [(N, K, sk) for N in (128, 256) for K, sk in ((128, 0), (256, 2),
                                                    (640, 2))]
ROWS = [1, 32, 33, 128, 129, 256, 257, 511, 512]


def wide_slices(N, K, splitk=0):
    """The documented slicing: whole groups, ceil(128 / panels) slices but
    at least 4 groups in a slice, ceil(groups / slices) groups per slice,
    no empty slice; ``forced_slices`` under a caller's ``splitk``."""
    sk = min(max(1, -(-128 // (N // 128))), max(1, K // GROUP // 4))
    sl = forced_slices(K, splitk or sk)
    assert ops.w4a16_wide_plan(N, K, splitk) == (len(sl), sl[0][1] - sl[0][0])
    return sl


def run(form, case, splitk=0, x=None, **kw):
    sm = case.meta if form == "zp" else case.s
    return getattr(ops, FORMS[form][1])(
        case.x.to(DEV) if x is None else x, case.packed.to(DEV), sm.to(DEV),
        splitk, **kw)


@forms
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("nk", NK, ids=lambda s: "x".join(map(str, s)))
def test_exact_integers_bit_equal_in_poisoned_surroundings(form, nk, M):
    """``out`` and x are the first M rows of NaN-filled buffers one row
    longer, the slab is NaN-filled: the result is bit-equal to the oracle
    (so finite), the row after ``out`` is untouched, the row after x is
    never read."""
    N, K, splitk = nk
    slices = wide_slices(N, K, splitk)
    assert len(slices) == (2 if splitk else 1)
    case = FORMS[form][0].exact_case(M, N, K, slices=slices)
    buf = torch.full((M + 1, N), NAN, dtype=BF16, device=DEV)
    xbuf = torch.full((M + 1, K), NAN, dtype=BF16, device=DEV)
    xbuf[:M] = case.x.to(DEV)
    ws = torch.full((len(slices) * M * N,), NAN, device=DEV)
    got = run(form, case, splitk, x=xbuf[:M], out=buf[:M], ws=ws)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got.cpu(), case.expected), describe(got.cpu(), case)
    assert bool(buf[M].isnan().all())


@forms
@pytest.mark.parametrize("M", [129, 512])
def test_needles_bit_equal(form, M):
    """One sweep holds 0, 7, 8, 31, 32, 127, 128, K-1 and both sides of the
    slice boundary."""
    N, K = 128, 1024
    slices = wide_slices(N, K)
    assert len(slices) == 2 and n_edge_sweeps(M, K, slices) == 1
    mod = FORMS[form][0]
    case = mod.needle_case(M, N, K, mod.needle_weights(N, K), slices=slices)
    out = run(form, case).cpu()
    assert torch.equal(out, case.expected), describe(out, case)


@forms
def test_rows_do_not_depend_on_M(form):
    case = FORMS[form][0].random_case(512, 128, 1024)
    full = run(form, case)
    part = run(form, case, x=case.x.to(DEV)[:129])
    assert torch.equal(bits(full[:129]), bits(part))


@forms
@pytest.mark.parametrize("shape", [(129, 128, 1024), (512, 256, 4096)],
                         ids=lambda s: "x".join(map(str, s)))
def test_random_bf16_within_the_existing_bound(form, shape):
    """|got - y64| <= 2^-8 |y64| + 2^-19 S, the bound of w4a16_linear."""
    mod = FORMS[form][0]
    case = mod.random_case(*shape)
    y, allowed, _ = mod.random_bound(case)
    err = (run(form, case).cpu().double() - y).abs()
    print(f"{form} wide random {shape}: max err/allowed "
          f"{float((err / allowed).max()):.3f}")
    assert bool((err <= allowed).all()), float((err / allowed).max())


@pytest.mark.parametrize("quant", ["int4", "int4-awq"])
def test_linear_w4_routes_listed_shapes_to_the_wide_op(quant, monkeypatch):
    """tiny-128's qkv shape listed for 257..512 rows: 300 rows give the
    wide op's bits and leave the dequant scratch untouched; inside
    forward_prefill's flag the scratch is written."""
    cfg = get_config("tiny-128")
    N, K = cfg.q_size + 2 * cfg.kv_size, cfg.hidden_size
    monkeypatch.setattr(LlamaForCausalLM, "_W4_WIDE_ROWS_BY_SHAPE",
                        {(N, K): (257, 512)})
    model = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=3, quant=quant)
    op, sfx = ((ops.w4a16_zp_wide_linear, ".m4") if quant == "int4-awq"
               else (ops.w4a16_wide_linear, ".s4"))
    x = torch.randn(300, K,
                    generator=torch.Generator().manual_seed(1)).to(BF16).to(DEV)
    model._w4_scratch.fill_(7.0)
    got = model._linear_w4(x, "l0.qkv")
    want = op(x, model.params["l0.qkv.q4"], model.params["l0.qkv" + sfx])
    assert torch.equal(bits(got), bits(want))
    assert bool((model._w4_scratch == 7.0).all())
    model._w4_tiled = False                 # as forward_prefill sets it
    model._linear_w4(x, "l0.qkv")
    assert not bool((model._w4_scratch == 7.0).all())


def test_argument_checks():
    case = w4a16_cases.exact_case(3, 128, 256)
    packed, s = case.packed.to(DEV), case.s.to(DEV)

    def x(M, K=256):
        return torch.zeros(M, K, dtype=BF16, device=DEV)
    ops.w4a16_wide_linear(x(512), packed, s)
    with pytest.raises(RuntimeError, match="N % 128"):
        ops.w4a16_wide_linear(x(3), packed[:64 * 256 // 8],
                              s[:64].contiguous())
    with pytest.raises(RuntimeError):                       # K = 64
        ops.w4a16_wide_linear(x(3, 64), packed[:128 * 64 // 8], s[:, :0])
    for M in (0, 513):
        with pytest.raises(RuntimeError, match="1 <= M <= 512"):
            ops.w4a16_wide_linear(x(M), packed, s)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.w4a16_wide_linear(x(3), packed, s,
                              out=torch.empty(2, 128, dtype=BF16, device=DEV))
    with pytest.raises(RuntimeError, match="slices\\*M\\*N"):
        ops.w4a16_wide_linear(x(3), packed, s, 2,
                              ws=torch.empty(8, device=DEV))
