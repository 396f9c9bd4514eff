"""Boundary-exact tests of the attention kernels (decode_attn.hip,
prefill_mfma.hip with its in-batch and paged entries, prefill_attn.hip,
rope_kv.hip).

Random inputs go blind with length: at the project's bf16 tolerance a
reference that attends to one key too many passes at L = 300.  These
tests use inputs whose answer is known exactly (tests/attn_boundary_cases.py):
a RAMP whose softmax is a one-hot on the last allowed key, a UNIFORM
fill where every key is worth exactly 1/L, and a NEEDLE sweep, with
finite poison in every slot a kernel must not read.

The first half runs on the CPU and is what gives the GPU half its
meaning: for every case list the comparator accepts the plain fp32
reference (ops/ref.py) and REJECTS deliberately wrong references — last
key dropped, one extra key, an interior key removed, causal mask shifted
by one.  No deliberately broken kernel is ever run on a GPU.

Poison is finite only (kernels.h: slots past seq_len must hold finite
values — a masked p = 0 still multiplies the loaded V).
"""

import math
import os

import pytest
import torch

import resilient_llm_amd.ops as ops
from resilient_llm_amd.ops import ref
from tests import attn_boundary_cases as C

DEV = "cuda"
BF16 = torch.bfloat16
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(C.FP8, id="fp8")]
KINDS = ["ramp", "uniform"]


def _id(shape):
    return "x".join(str(s) for s in shape)


def deq(cache):
    """What a cache holds, as bf16 (exact for fp8: e4m3 is a subset)."""
    return cache.float().to(BF16)


def raw(t):
    """Bit pattern of a bf16 / fp8 tensor, for bit-exact comparisons."""
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def check(got, want, kind, n_keys, what, labels=None):
    """Assert through THE comparator; name the offending rows."""
    atol, rtol = C.tolerances(kind, n_keys)
    bad = C.bad_rows(got.cpu(), want, atol, rtol)
    if bad.any():
        idx = bad.nonzero().flatten().tolist()
        lab = labels if labels is not None else n_keys
        err = (got.cpu().double().reshape(len(bad), -1)
               - want.double().reshape(len(bad), -1)).abs().amax(1)
        raise AssertionError(
            f"{what}: {len(idx)} rows outside tolerance; (row, keys, max err) "
            + str([(i, int(lab[i]), float(err[i])) for i in idx[:12]]))


def assert_power(kind, D, n_keys, limit, correct, what):
    """The comparator accepts the correct reference and the closed form,
    and rejects every wrong reference the construction must catch, on
    every row where that wrong reference exists."""
    want = C.attend(kind, D, C.allowed_upto(n_keys))
    R = len(n_keys)
    if kind == "ramp":
        # closed form: exactly V[last allowed key], zero for no key
        last = C.ramp_v((n_keys - 1).clamp_min(0), D) \
            * (n_keys > 0).unsqueeze(1)
        # float64: the neighbour weighs exp(-c/sqrt(D)) = 1.13e-7 and its
        # V differs by at most 10
        assert (want - last).abs().max() <= 1.2e-6
    atol, rtol = C.tolerances(kind, n_keys)
    for name, got in correct.items():
        got = got.reshape(R, -1, D)
        w = want.unsqueeze(1).expand_as(got)
        if kind == "ramp":
            # the bf16 reference output: exact but for 7 * 1.13e-7 where
            # V[t*] is 0 (its neighbour is -7 there)
            assert (got.double() - last.unsqueeze(1)).abs().max() <= 8e-7
        assert not C.bad_rows(got, w, atol, rtol).any(), (what, name)
    for name in C.CATCHES[kind]:
        allowed, defined = C.mutant(name, n_keys, limit)
        assert defined.any(), (what, name)
        wrong = C.attend(kind, D, allowed)
        flagged = C.bad_rows(wrong, want, atol, rtol)
        missed = (defined & ~flagged).nonzero().flatten().tolist()
        assert not missed, (
            f"{what}: comparator cannot tell '{name}' from the truth for "
            f"rows with n_keys {[int(n_keys[i]) for i in missed[:12]]}")
        assert not (flagged & ~defined).any()


# =========================================================== CPU: power
def test_codes_exact_in_bf16_and_e4m3():
    for D in (64, 128):
        for kind in KINDS:
            v = C.value_table(kind, D)
            assert torch.equal(v.to(BF16).float(), v)
            assert torch.equal(v.to(C.FP8).float(), v)
        k = C.ramp_k(torch.arange(C.SPARE + 1), D)
        assert torch.equal(k.to(C.FP8).float(), k)
        q = C.ramp_q(D)
        assert torch.equal(q.to(BF16).float(), q)
        # adjacent scores are ~16 apart: the neighbour weighs < 2e-7
        assert abs(C.ramp_c(D) / math.sqrt(D) - 16) < 0.01


def test_decode_lens_cover_the_edges():
    need = {0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193,
            255, 256, 257, 271}
    for batch, *_ in C.DECODE_SHAPES:
        seen = set()
        for lens in C.decode_launches(batch):
            assert len(lens) == batch
            seen |= set(lens.tolist())
        assert need <= seen
        for m in range(16, 257, 16):
            assert {m - 1, m, m + 1} <= seen
        assert 0 not in torch.cat(C.decode_launches(batch, fused=True)).tolist()
    # chains of 1..5 blocks per wave at split 1 (block stride 4)
    assert {(l + 15) // 16 for l in C.DECODE_LENS} >= set(range(1, 18))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", C.DECODE_SHAPES, ids=_id)
def test_power_decode(shape, kind):
    batch, n_q, n_kv, D, _ = shape
    kc, vc, table, spare = C.paged_cache(kind, batch, n_kv, D)
    q = C.query_rows(kind, batch, n_q, D)
    limit = torch.full((batch,), C.SPARE)
    caches = {dt: (deq(kc.to(dt)), deq(vc.to(dt))) for dt in (BF16, C.FP8)}
    for lens in C.decode_launches(batch):
        bt = C.block_table(table, lens, spare)
        correct = {dt: ref.decode_attn(q, k, v, bt, lens.int(),
                                       1 / math.sqrt(D))
                   for dt, (k, v) in caches.items()}
        assert_power(kind, D, lens, limit, correct, f"decode {shape}")


@pytest.mark.parametrize("shape", C.DECODE_SHAPES, ids=_id)
def test_power_needle(shape):
    """Every position 0..L-1 is a needle in some launch; ref.decode_attn
    is the sweep's reference, and a reference that loses the target key
    (every launch, every row) or the last key is rejected."""
    batch, n_q, n_kv, D, n_split = shape
    kc, vc, bt, lens, rounds = C.needle_case(*shape)
    L = int(lens[0])
    assert (L + 15) // 16 >= 3 * 4 * n_split        # >= 3 blocks per chain
    assert set(torch.cat(rounds).flatten().tolist()) == set(range(L))
    scale = 1 / math.sqrt(D)
    tol = (C.BF16_TOL, C.BF16_TOL)
    seen_last = False
    for targets in rounds:
        q = C.needle_queries(kc, bt, targets)
        want = ref.decode_attn(q, kc, vc, bt, lens, scale)
        ok = C.decode_oracle(q, kc, vc, bt, lens, scale)
        assert not C.bad_rows(ok, want, *tol).any()
        lost = C.decode_oracle(q, kc, vc, bt, lens, scale, drop=targets)
        # per needle, not per sequence: each (sequence, head) must show it
        assert C.bad_rows(lost.reshape(-1, D), want.reshape(-1, D), *tol).all()
        has_last = (targets == L - 1).flatten()
        if has_last.any():
            seen_last = True
            short = C.decode_oracle(q, kc, vc, bt, lens - 1, scale)
            assert C.bad_rows(short.reshape(-1, D), want.reshape(-1, D),
                              *tol)[has_last].all()
    assert seen_last


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", C.PREFILL_SHAPES, ids=_id)
def test_power_prefill(shape, kind):
    n_q, n_kv, D = shape
    pos, own, cu = C.prefill_positions()
    qkv = C.prefill_qkv(kind, n_q, n_kv, D)
    T = len(pos)
    q = qkv[:, :n_q * D].reshape(T, n_q, D)
    k = qkv[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D)
    v = qkv[:, (n_q + n_kv) * D:].reshape(T, n_kv, D)
    out = ref.prefill_attn(q, k, v, cu, 1 / math.sqrt(D))
    # causal mask shifted by -1 / +1 == drop_last / one_extra per row
    assert_power(kind, D, pos + 1, own, {"ref": out}, f"prefill {shape}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", C.PAGED_SHAPES, ids=_id)
def test_power_prefill_paged(shape, kind):
    n_q, n_kv, D = shape
    ch = C.paged_chunks()
    assert ch["n_tables"] >= 3
    kc, vc, table, spare = C.paged_cache(kind, ch["n_tables"], n_kv, D)
    bt = C.block_table(table, ch["kv_hi"], spare)
    qkv = C.paged_qkv(kind, ch["T"], n_q, n_kv, D)
    correct = {}
    for dt in (BF16, C.FP8):
        out = ref.prefill_paged_attn(
            qkv, deq(kc.to(dt)), deq(vc.to(dt)), ch["row0"], ch["pos0"],
            ch["nrows"], ch["btrow"], bt, 1 / math.sqrt(D), n_q)
        correct[dt] = out[ch["rows"]]
    limit = torch.full((len(ch["rows"]),), C.SPARE)
    assert_power(kind, D, ch["pos"] + 1, limit, correct, f"paged {shape}")


# ================================================================== GPU
def _split(batch, n_kv):
    ops.load_extension(required=True)
    return int(torch.ops.rlli.decode_attn_split(batch, n_kv))


@pytest.fixture
def split_env():
    for var in ("RLLI_ATTN_SPLIT", "RLLI_NO_SPLITK"):
        if var in os.environ:
            pytest.skip(f"{var} is set: it overrides the decode split "
                        "factor these cases are built to cover")


def _with_kv_poison(q, n_kv, D):
    """[B, (n_q + 2 n_kv) D] qkv whose k/v columns hold the spare code
    (decode_attn_qkv must read only the q columns)."""
    B = q.shape[0]
    kv = torch.full((B, 2 * n_kv * D), C.SPARE_V, dtype=BF16, device=q.device)
    return torch.cat([q.reshape(B, -1), kv], dim=1).contiguous()


def _decode_both(q, kc, vc, bt, lens, scale, n_kv):
    B, n_q, D = q.shape
    a = ops.decode_attn(q, kc, vc, bt, lens, scale)
    b = ops.decode_attn_qkv(_with_kv_poison(q, n_kv, D), kc, vc, bt, lens,
                            scale, n_q)
    return {"decode_attn": a, "decode_attn_qkv": b.reshape(B, n_q, D)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.DECODE_SHAPES, ids=_id)
def test_decode_boundaries(shape, dtype, kind, split_env):
    batch, n_q, n_kv, D, n_split = shape
    assert _split(batch, n_kv) == n_split
    kc, vc, table, spare = C.paged_cache(kind, batch, n_kv, D, dtype)
    kc, vc = kc.to(DEV), vc.to(DEV)
    q = C.query_rows(kind, batch, n_q, D).to(DEV)
    for lens in C.decode_launches(batch):
        bt = C.block_table(table, lens, spare).to(DEV)
        want = C.attend(kind, D, C.allowed_upto(lens))
        outs = _decode_both(q, kc, vc, bt, lens.int().to(DEV),
                            1 / math.sqrt(D), n_kv)
        for name, out in outs.items():
            check(out, want.unsqueeze(1).expand(batch, n_q, D), kind, lens,
                  f"{name} {kind} split {n_split}")
            empty = out.cpu()[lens == 0]
            assert (empty == 0).all(), f"{name}: seq_len 0 must give zeros"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.DECODE_SHAPES, ids=_id)
def test_decode_needle_sweep(shape, dtype, split_env):
    """Every position 0..L-1 of a sequence long enough for three blocks
    per wave chain is the needle of some (sequence, head): one launch
    where batch * n_q >= L, successive launches on the same cache where
    it is not (2 at split 3, 97 at split 16)."""
    batch, n_q, n_kv, D, n_split = shape
    assert _split(batch, n_kv) == n_split
    kc, vc, bt, lens, rounds = C.needle_case(*shape, dtype=dtype)
    scale = 1 / math.sqrt(D)
    kc_r, vc_r = deq(kc), deq(vc)
    dev = [t.to(DEV) for t in (kc, vc, bt, lens)]
    for targets in rounds:
        q = C.needle_queries(kc, bt, targets)
        want = ref.decode_attn(q, kc_r, vc_r, bt, lens, scale)
        outs = _decode_both(q.to(DEV), *dev, scale, n_kv)
        for name, out in outs.items():
            bad = C.bad_rows(out.cpu().reshape(batch * n_q, D),
                             want.reshape(batch * n_q, D),
                             C.BF16_TOL, C.BF16_TOL)
            assert not bad.any(), (
                f"{name} split {n_split}: needle lost at positions "
                f"{sorted(set(targets.flatten()[bad].tolist()))[:24]}")


FUSED_SHAPES = [s for s in C.DECODE_SHAPES if s[:4] in ((48, 32, 8, 128),
                                                        (4, 8, 2, 64))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=_id)
def test_decode_fused_ramp(shape, dtype, split_env):
    """decode_attn_rope_qkv: the new token's k/v arrive in qkv and its
    cache slot holds the spare code beforehand.  The output is V[len-1]
    (the stale slot would give the spare code, a dropped self term
    V[len-2]); afterwards the slot holds exactly the new k/v and no other
    byte of either cache has changed."""
    batch, n_q, n_kv, D, n_split = shape
    assert _split(batch, n_kv) == n_split
    kc32, vc32, table, spare = C.paged_cache("ramp", batch, n_kv, D,
                                             torch.float32)
    kc0, vc0 = kc32.to(dtype), vc32.to(dtype)           # pristine ramp
    cs = C.identity_rope(C.SPARE, D).to(DEV)
    rows = torch.arange(batch)
    for lens in C.decode_launches(batch, fused=True):
        new = lens - 1                                  # position appended
        phys = table.long()[rows, new // C.BS]
        kc, vc = kc32.clone(), vc32.clone()
        kc[phys, :, new % C.BS] = C.ramp_k(torch.tensor([C.SPARE]), D)
        vc[phys, :, new % C.BS] = C.SPARE_V
        kc, vc = kc.to(dtype), vc.to(dtype)
        before_k, before_v = kc.clone(), vc.clone()
        kc, vc = kc.to(DEV), vc.to(DEV)
        qkv = torch.cat([
            C.query_rows("ramp", batch, n_q, D).reshape(batch, -1).float(),
            C.ramp_k(new, D).repeat(1, n_kv),
            C.ramp_v(new, D).repeat(1, n_kv)], dim=1).to(BF16).to(DEV)
        slots = (phys * C.BS + new % C.BS).int()
        out = ops.decode_attn_rope_qkv(
            qkv, new.int().to(DEV), cs, kc, vc, slots.to(DEV),
            C.block_table(table, lens, spare).to(DEV), lens.int().to(DEV),
            1 / math.sqrt(D), n_q)
        want = C.attend("ramp", D, C.allowed_upto(lens))
        check(out.reshape(batch, n_q, D),
              want.unsqueeze(1).expand(batch, n_q, D), "ramp", lens,
              f"decode_attn_rope_qkv split {n_split}")
        kc, vc = kc.cpu(), vc.cpu()
        # the slot now holds exactly the new k/v ...
        assert torch.equal(kc.float()[phys, :, new % C.BS],
                           C.ramp_k(new, D).unsqueeze(1).expand(-1, n_kv, -1))
        assert torch.equal(vc.float()[phys, :, new % C.BS],
                           C.ramp_v(new, D).unsqueeze(1).expand(-1, n_kv, -1))
        # ... and nothing else changed: bit-identical outside the slots
        touched = torch.zeros(kc.shape[0], C.BS, dtype=torch.bool)
        touched[phys, new % C.BS] = True
        keep = ~touched[:, None, :, None].expand_as(kc)
        assert torch.equal(raw(kc)[keep], raw(before_k)[keep])
        assert torch.equal(raw(vc)[keep], raw(before_v)[keep])
        assert torch.equal(raw(kc), raw(kc0)) and torch.equal(raw(vc), raw(vc0))


@pytest.mark.gpu
def test_decode_fused_vs_unfused_at_split_1(split_env):
    """The random fused-vs-unfused comparison of test_ops_gpu.py at the
    serving shape, so the real rope runs on the split factor 1 path."""
    torch.manual_seed(11)
    B, n_q, n_kv, D, bs = 48, 32, 8, 128, 16
    assert _split(B, n_kv) == 1
    lens = C.decode_launches(B, fused=True)[0].tolist()
    width = (n_q + 2 * n_kv) * D
    nbt = max((l + bs - 1) // bs for l in lens)
    kc = torch.randn(B * nbt + 2, n_kv, bs, D, dtype=BF16, device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.randperm(B * nbt + 2)[:B * nbt].int().reshape(B, nbt).to(DEV)
    qkv = torch.randn(B, width, dtype=BF16, device=DEV)
    pos = torch.tensor([l - 1 for l in lens], dtype=torch.int32, device=DEV)
    slots = torch.tensor([int(bt[i, (l - 1) // bs]) * bs + (l - 1) % bs
                          for i, l in enumerate(lens)],
                         dtype=torch.int32, device=DEV)
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cs = ops.build_cos_sin(512, D, device=DEV)
    scale = 1.0 / math.sqrt(D)
    qkv_u, kc_u, vc_u = qkv.clone(), kc.clone(), vc.clone()
    ops.rope_kv_append_qkv_(qkv_u, pos, cs, kc_u, vc_u, slots, n_q)
    out_u = ops.decode_attn_qkv(qkv_u, kc_u, vc_u, bt, seq_lens, scale, n_q)
    out_f = ops.decode_attn_rope_qkv(qkv, pos, cs, kc, vc, slots, bt,
                                     seq_lens, scale, n_q)
    torch.testing.assert_close(out_f.float(), out_u.float(),
                               atol=C.BF16_TOL, rtol=C.BF16_TOL)
    torch.testing.assert_close(kc.float(), kc_u.float())
    torch.testing.assert_close(vc.float(), vc_u.float())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", C.PREFILL_SHAPES, ids=_id)
def test_prefill_boundaries(shape, kind):
    """prefill_attn_qkv (MFMA) and prefill_attn (VALU) on one ragged
    batch: row t of a sequence gives V[t] (ramp) / count/(t+1)."""
    n_q, n_kv, D = shape
    pos, _, cu = C.prefill_positions()
    T = len(pos)
    qkv = C.prefill_qkv(kind, n_q, n_kv, D).to(DEV)
    cu = cu.to(DEV)
    scale = 1 / math.sqrt(D)
    q = qkv[:, :n_q * D].reshape(T, n_q, D).contiguous()
    k = qkv[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D).contiguous()
    v = qkv[:, (n_q + n_kv) * D:].reshape(T, n_kv, D).contiguous()
    want = C.attend(kind, D, C.allowed_upto(pos + 1)) \
        .unsqueeze(1).expand(T, n_q, D)
    outs = {"prefill_attn_qkv":
            ops.prefill_attn_qkv(qkv, cu, scale, n_q, n_kv, D)
            .reshape(T, n_q, D),
            "prefill_attn": ops.prefill_attn(q, k, v, cu, scale)}
    for name, out in outs.items():
        check(out, want, kind, pos + 1, f"{name} {kind}")


def _paged_args(ch):
    return [ch[n].to(DEV) for n in ("row0", "pos0", "nrows", "btrow")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.PAGED_SHAPES, ids=_id)
def test_prefill_paged_boundaries(shape, dtype, kind):
    n_q, n_kv, D = shape
    ch = C.paged_chunks()
    kc, vc, table, spare = C.paged_cache(kind, ch["n_tables"], n_kv, D, dtype)
    bt = C.block_table(table, ch["kv_hi"], spare).to(DEV)
    qkv = C.paged_qkv(kind, ch["T"], n_q, n_kv, D).to(DEV)
    out = ops.prefill_paged_attn(qkv, kc.to(DEV), vc.to(DEV),
                                 *_paged_args(ch), bt, 1 / math.sqrt(D), n_q)
    R = len(ch["rows"])
    want = C.attend(kind, D, C.allowed_upto(ch["pos"] + 1))
    check(out.cpu()[ch["rows"]].reshape(R, n_q, D),
          want.unsqueeze(1).expand(R, n_q, D), kind, ch["pos"] + 1,
          f"prefill_paged_attn {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.PAGED_SHAPES, ids=_id)
def test_prefill_paged_random_vs_ref(shape, dtype):
    """Random data on the same chunk geometry against the fp32
    reference (fp8 -> bf16 staging is exact, so one tolerance)."""
    n_q, n_kv, D = shape
    ch = C.paged_chunks()
    g = torch.Generator().manual_seed(5)
    n_phys = ch["n_tables"] * C.N_TBL + 1
    kc = torch.randn(n_phys, n_kv, C.BS, D, generator=g).to(dtype)
    vc = torch.randn(n_phys, n_kv, C.BS, D, generator=g).to(dtype)
    bt = torch.randperm(n_phys, generator=g)[:-1] \
        .reshape(ch["n_tables"], C.N_TBL).int().contiguous()
    qkv = torch.randn(ch["T"], (n_q + 2 * n_kv) * D, generator=g).to(BF16)
    scale = 1 / math.sqrt(D)
    want = ref.prefill_paged_attn(qkv, deq(kc), deq(vc), ch["row0"],
                                  ch["pos0"], ch["nrows"], ch["btrow"], bt,
                                  scale, n_q)
    out = ops.prefill_paged_attn(qkv.to(DEV), kc.to(DEV), vc.to(DEV),
                                 *_paged_args(ch), bt.to(DEV), scale, n_q)
    check(out.cpu()[ch["rows"]], want[ch["rows"]], "needle", ch["pos"] + 1,
          "prefill_paged_attn random")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", C.PREFILL_SHAPES, ids=_id)
def test_prefill_entries_agree_bitwise(shape):
    """prefill_attn_qkv and prefill_paged_attn share one tile body, so on
    a bf16 cache that holds the batch's own K/V (the bf16 codec is the
    identity) they give the same bits for every row."""
    n_q, n_kv, D = shape
    _, _, cu = C.prefill_positions()
    T = int(cu[-1])
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(T, (n_q + 2 * n_kv) * D, generator=g).to(BF16)
    kc, vc, bt, ch = C.prefill_as_paged(qkv, n_q, n_kv, D)
    covered = torch.zeros(T, dtype=torch.int64)
    for r0, n in zip(ch["row0"].tolist(), ch["nrows"].tolist()):
        assert 1 <= n <= 32
        covered[r0:r0 + n] += 1
    assert (covered == 1).all(), "chunks must cover every row exactly once"
    scale = 1 / math.sqrt(D)
    batch = ops.prefill_attn_qkv(qkv.to(DEV), cu.to(DEV), scale, n_q, n_kv, D)
    paged = ops.prefill_paged_attn(qkv.to(DEV), kc.to(DEV), vc.to(DEV),
                                   *_paged_args(ch), bt.to(DEV), scale, n_q)
    differ = (raw(batch.cpu()) != raw(paged.cpu())).any(dim=1)
    assert not differ.any(), (
        f"{int(differ.sum())} rows differ in their bits, first "
        f"{differ.nonzero().flatten().tolist()[:12]}")


@pytest.mark.gpu
@pytest.mark.parametrize("fused_qkv", [False, True], ids=["qkv3", "qkv"])
@pytest.mark.parametrize("shape", [(32, 8, 128), (4, 2, 64)], ids=_id)
def test_rope_kv_append_fp8_cache(shape, fused_qkv):
    """rope_kv_append_ / rope_kv_append_qkv_ into an fp8 cache with some
    slot == -1 tokens: written slots dequantise to within one e4m3 step
    of the bf16 result (6.25 % + the smallest e4m3 step), every other
    slot is bit-identical to before, and q/k are rotated for the skipped
    tokens too."""
    n_q, n_kv, D = shape
    T, blocks, bs = 11, 6, 16
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(T, (n_q + 2 * n_kv) * D, generator=g).to(BF16)
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    cs = ops.build_cos_sin(512, D)
    slots = (torch.arange(3, 3 + T) * 7 % (blocks * bs)).int()
    slots[[0, 4, T - 1]] = -1
    kc0 = torch.randn(blocks, n_kv, bs, D, generator=g).to(C.FP8)
    vc0 = torch.randn(blocks, n_kv, bs, D, generator=g).to(C.FP8)

    def split3(x):
        return (x[:, :n_q * D].reshape(T, n_q, D).contiguous(),
                x[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D).contiguous(),
                x[:, (n_q + n_kv) * D:].reshape(T, n_kv, D).contiguous())

    # bf16 result on the CPU reference (cache at bf16 precision)
    q_r, k_r, v_r = split3(qkv.clone())
    kc_r, vc_r = deq(kc0), deq(vc0)
    ref.rope_kv_append_(q_r, k_r, v_r, pos, cs, kc_r, vc_r, slots)

    kc, vc = kc0.clone().to(DEV), vc0.clone().to(DEV)
    if fused_qkv:
        x = qkv.clone().to(DEV)
        ops.rope_kv_append_qkv_(x, pos.to(DEV), cs.to(DEV), kc, vc,
                                slots.to(DEV), n_q)
        q_g, k_g, v_g = split3(x.cpu())
    else:
        q_g, k_g, v_g = (t.to(DEV) for t in split3(qkv.clone()))
        ops.rope_kv_append_(q_g, k_g, v_g, pos.to(DEV), cs.to(DEV), kc, vc,
                            slots.to(DEV))
    for got, want in ((q_g, q_r), (k_g, k_r)):          # skipped ones too
        torch.testing.assert_close(got.cpu().float(), want.float(),
                                   atol=C.BF16_TOL, rtol=C.BF16_TOL)
    assert torch.equal(raw(v_g.cpu()), raw(v_r))        # v is only read
    written = torch.zeros(blocks, bs, dtype=torch.bool)
    ok = slots >= 0
    written[slots[ok].long() // bs, slots[ok].long() % bs] = True
    assert int(written.sum()) == T - 3
    w = written[:, None, :, None].expand_as(kc0)
    for got, before, want in ((kc.cpu(), kc0, kc_r), (vc.cpu(), vc0, vc_r)):
        assert torch.equal(raw(got)[~w], raw(before)[~w])
        err = (got.float() - want.float()).abs()
        tol = want.float().abs() * 0.0625 + 2.0 ** -9
        assert (err <= tol)[w].all(), float((err - tol)[w].max())
