"""Qwen3 q/k norm on the GPU: ops.qk_norm_rope_kv_append_qkv_ and
ops.decode_attn_qknorm_rope_qkv against float64, the tiny-qk-128 model
against its float32 CPU twin, and the wrappers' rejections.

Norm weights are 1 + 0.25 * randn everywhere (with ones a dropped weight
multiply would pass).  What the kernels must not read is NaN: cache blocks
nobody owns (block-table padding points at one) and qkv rows beyond the
batch.  The split-K workspace is allocated inside the op, so a test cannot
poison it; the split cases check its use through the result.  The slots of a
sequence's last block past seq_len hold the cache dtype's largest finite
value instead: decode_attn's contract (kernels.h) is that masked slots are
finite, because their V is multiplied by p = 0; any weight above 0 on such
a slot still wrecks the answer."""

import pytest
import torch

from attn_boundary_cases import BF16_TOL, BS, FP8, bad_rows, decode_oracle
from qk_norm_cases import norm_rope64
from resilient_llm_amd import ops
from resilient_llm_amd.engine import PagedKVCache
from resilient_llm_amd.models import LlamaForCausalLM, get_config
from resilient_llm_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
NAN = float("nan")
EPS = 1e-6


def make_qkv(T, n_q, n_kv, D, g):
    """(qkv [T + 2, W] bf16 whose last two rows are NaN, wq, wk)."""
    qkv = torch.full((T + 2, (n_q + 2 * n_kv) * D), NAN, dtype=BF16)
    qkv[:T] = (2 * torch.randn(T, qkv.shape[1], generator=g)).to(BF16)
    wq = (1 + 0.25 * torch.randn(D, generator=g)).to(BF16)
    wk = (1 + 0.25 * torch.randn(D, generator=g)).to(BF16)
    return qkv, wq, wk


def split_heads(x, n_q, n_kv, D):
    return [t.reshape(x.shape[0], -1, D) for t in
            x.split([n_q * D, n_kv * D, n_kv * D], dim=1)]


def rope_bound(x, w, pos, cs):
    """(want, bound) of out = n1 c -+ n2 s in float64: 2^-8 (|n1 c| +
    |n2 s|) + 2^-20."""
    n, want = norm_rope64(x, w, EPS, pos, cs)
    half = x.shape[-1] // 2
    c = cs.double()[pos.long()][:, None, :]
    nc = (n * torch.cat([c[..., :half], c[..., :half]], -1)).abs()
    ns = (torch.cat([n[..., half:], n[..., :half]], -1)
          * torch.cat([c[..., half:], c[..., half:]], -1)).abs()
    return want, 2.0 ** -8 * (nc + ns) + 2.0 ** -20


def e4m3_step(x):
    """Spacing of e4m3 at |x| (2^-9 below the smallest normal 2^-6)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -6)))
    return torch.exp2(e - 3)


def check_slot(kc, vc, slot, k_out, v_in, what):
    """Cache row ``slot`` against the bf16 k written in place and the v."""
    krow = kc[slot // BS, :, slot % BS].float()
    vrow = vc[slot // BS, :, slot % BS].float()
    if kc.dtype == FP8:
        k8 = k_out.to(FP8).float()
        assert ((krow - k8).abs() <= e4m3_step(k8)).all(), what
        assert torch.equal(vrow, v_in.to(FP8).float()), what
    else:
        assert torch.equal(krow, k_out.float()), what
        assert torch.equal(vrow, v_in.float()), what


@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n_q,n_kv", [(4, 1), (8, 2), (32, 8)])
@pytest.mark.parametrize("D", [64, 128])
def test_unfused_against_float64(D, n_q, n_kv, T, cache_dtype):
    """q and k within 2^-8 (|n1 c| + |n2 s|) + 2^-20 of float64: the one
    bf16 rounding of the rotated value (2^-8 relative, round to nearest on
    8 significand bits) plus f32 noise.  A second rounding of n before the
    rotation would use up to twice that."""
    g = torch.Generator().manual_seed(D + n_q + T)
    qkv, wq, wk = make_qkv(T, n_q, n_kv, D, g)
    pos = torch.tensor([37, 0, 5][:T], dtype=torch.int32)
    slots = torch.tensor([35, -1, 2][:T], dtype=torch.int32)
    cs = ref.build_cos_sin(64, D, 1e6)
    kc = torch.full((3, n_kv, BS, D), NAN).to(cache_dtype).to(DEV)
    vc = kc.clone()
    x = qkv.to(DEV)
    ops.qk_norm_rope_kv_append_qkv_(x[:T], wq.to(DEV), wk.to(DEV), EPS,
                                    pos.to(DEV), cs.to(DEV), kc, vc,
                                    slots.to(DEV), n_q)
    x, kc, vc = x.cpu(), kc.cpu(), vc.cpu()
    assert x[T:].isnan().all()
    q0, k0, v0 = split_heads(qkv[:T], n_q, n_kv, D)
    q, k, v = split_heads(x[:T], n_q, n_kv, D)
    assert torch.equal(v, v0)
    untouched = torch.ones(3 * BS, dtype=torch.bool)
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            untouched[s] = False
            check_slot(kc, vc, s, k[t], v0[t], f"token {t}")
    for c in (kc, vc):
        rows = c.float().transpose(1, 2).reshape(3 * BS, -1)
        assert rows[untouched].isnan().all() and not rows[~untouched].isnan().any()
    for name, got, x0, w in (("q", q, q0, wq), ("k", k, k0, wk)):
        want, bound = rope_bound(x0, w, pos, cs)
        err = (got.double() - want).abs()
        print(f"{name}: max err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), name


def decode_case(D, group, batch, cache_dtype, seed):
    """A batch whose rows cycle through seq_len 1, 16, 17, 33.  Returns the
    op's inputs on the CPU and the oracle's answer."""
    g = torch.Generator().manual_seed(seed)
    n_kv, n_q = 2, 2 * group
    lens = torch.tensor([[1, 16, 17, 33][r % 4] for r in range(batch)],
                        dtype=torch.int32)
    nb = 3
    perm = torch.randperm(batch * nb + 1, generator=g)
    poison = int(perm[-1])
    bt = perm[:-1].reshape(batch, nb).to(torch.int32)
    kc = torch.randn(batch * nb + 1, n_kv, BS, D, generator=g)
    vc = torch.randn(batch * nb + 1, n_kv, BS, D, generator=g)
    kc, vc = kc.to(cache_dtype), vc.to(cache_dtype)
    qkv, wq, wk = make_qkv(batch, n_q, n_kv, D, g)
    pos = lens - 1
    cs = ref.build_cos_sin(64, D, 1e6)
    q0, k0, v0 = split_heads(qkv[:batch], n_q, n_kv, D)
    # head 0 of every row looks for the appended token: q = 3 k_new before
    # the norm, so after it q_n . k_n is ~D * w_q w_k against ~sqrt(D)
    q0[:, 0] = 3 * k0[:, 0]
    qkv[:batch, :D] = q0[:, 0]
    _, qr = norm_rope64(q0, wq, EPS, pos, cs)
    _, kr = norm_rope64(k0, wk, EPS, pos, cs)
    last = bt.long().gather(1, (pos // BS).long()[:, None])[:, 0]
    # oracle cache: the float64 k of the new token at cache precision
    kc_o, vc_o = kc.float(), vc.float()
    kc_o[last, :, (pos % BS).long()] = kr.float().to(cache_dtype).float()
    vc_o[last, :, (pos % BS).long()] = v0.to(cache_dtype).float()
    want = decode_oracle(qr, kc_o, vc_o, bt, lens, D ** -0.5)
    # poison: the unowned block and table padding NaN, masked slots huge
    big = torch.finfo(cache_dtype).max
    kc_p, vc_p = kc.float(), vc.float()
    for c in (kc_p, vc_p):
        c[poison] = NAN
        for r in range(batch):
            c[last[r], :, int(pos[r]) % BS:] = big
            c[bt[r, int(pos[r]) // BS + 1:].long()] = NAN
    bt_p = bt.clone()
    for r in range(batch):
        bt_p[r, int(pos[r]) // BS + 1:] = poison
    slots = (last * BS + (pos % BS).long()).to(torch.int32)
    return dict(qkv=qkv, wq=wq, wk=wk, pos=pos, cs=cs,
                kc=kc_p.to(cache_dtype), vc=vc_p.to(cache_dtype),
                slots=slots, bt=bt_p, lens=lens, n_q=n_q, n_kv=n_kv,
                k0=k0, v0=v0), want


@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("batch", [4, 192])
@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_fused_decode_against_oracle(D, group, batch, cache_dtype):
    ops.load_extension(required=True)
    c, want = decode_case(D, group, batch, cache_dtype, D + group + batch)
    n_split = torch.ops.rlli.decode_attn_split(batch, c["n_kv"])
    assert (n_split == 1) == (batch == 192)
    d = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v
         for k, v in c.items()}
    kc_f, vc_f = d["kc"].clone(), d["vc"].clone()
    got = ops.decode_attn_qknorm_rope_qkv(
        d["qkv"][:batch], d["wq"], d["wk"], EPS, d["pos"], d["cs"], kc_f,
        vc_f, d["slots"], d["bt"], d["lens"], D ** -0.5, c["n_q"])
    got = got.cpu().view(batch, c["n_q"], D)
    err = (got.double() - want).abs().max().item()
    print(f"n_split {n_split}: max abs err {err:.3e}")
    bad = bad_rows(got, want, BF16_TOL, BF16_TOL)
    assert not bad.any(), (bad.nonzero().flatten().tolist(), err)
    # the appended slot: what the unfused op writes for the same token
    kc_u, vc_u = d["kc"].clone(), d["vc"].clone()
    x = d["qkv"].clone()
    ops.qk_norm_rope_kv_append_qkv_(x[:batch], d["wq"], d["wk"], EPS,
                                    d["pos"], d["cs"], kc_u, vc_u,
                                    d["slots"], c["n_q"])
    _, k_u, _ = split_heads(x[:batch].cpu(), c["n_q"], c["n_kv"], D)
    _, bound = rope_bound(c["k0"], c["wk"], c["pos"], c["cs"])
    kc_f, vc_f, kc_u, vc_u = (t.cpu() for t in (kc_f, vc_f, kc_u, vc_u))
    for r, s in enumerate(c["slots"].tolist()):
        check_slot(kc_u, vc_u, s, k_u[r], c["v0"][r], f"unfused row {r}")
        kf = kc_f[s // BS, :, s % BS].float()
        ku = kc_u[s // BS, :, s % BS].float()
        if cache_dtype == FP8:
            assert ((kf - ku).abs() <= e4m3_step(ku)).all(), r
        else:
            assert ((kf - ku).abs().double() <= bound[r]).all(), r
        assert torch.equal(vc_f[s // BS, :, s % BS].float(),
                           vc_u[s // BS, :, s % BS].float())
    # nothing but the appended slots changed
    for a, b in ((kc_f, c["kc"]), (vc_f, c["vc"])):
        rows_a = a.float().transpose(1, 2).reshape(-1, c["n_kv"] * D)
        rows_b = b.float().transpose(1, 2).reshape(-1, c["n_kv"] * D)
        keep = torch.ones(rows_a.shape[0], dtype=torch.bool)
        keep[c["slots"].long()] = False
        assert torch.equal(rows_a[keep].nan_to_num(7.0),
                           rows_b[keep].nan_to_num(7.0))


# ------------------------------------------------------------------ model
def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _set_norms(model, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    for i in range(cfg.n_layers):
        for n in ("q_norm", "k_norm"):
            if cfg.qk_norm:
                w = (1 + 0.25 * torch.randn(cfg.head_dim, generator=g))
                model.params[f"l{i}.{n}"] = w.to(model.dtype).to(model.device)


def _twin(gpu_model, cfg):
    twin = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=0)
    twin.params = {k: v.detach().cpu().float()
                   for k, v in gpu_model.params.items()}
    twin.cos_sin = gpu_model.cos_sin.cpu()
    return twin


def _steps(model, cfg, dev, graph=False):
    """Logits of a prefill (20 + 33 tokens), a mixed step (one decode row
    + a 5-token chunk of a third sequence) and a decode step of the two;
    with ``graph`` the decode step again, replayed three times."""
    f32 = model.dtype == torch.float32
    kv = PagedKVCache.for_model(cfg, 13, device=dev)
    if f32:
        kv.k, kv.v = kv.k.float(), kv.v.float()
    lens, toks, pos, slots, cu = [20, 33], [], [], [], [0]
    for b, n in enumerate(lens):
        toks += [(7 * b + 3 * t + 1) % cfg.vocab_size for t in range(n)]
        pos += list(range(n))
        slots += [b * 4 * BS + t for t in range(n)]
        cu.append(cu[-1] + n)
    i32 = lambda v: _i32(v, dev)
    out = [model.forward_prefill(i32(toks), i32(pos), kv, i32(slots), i32(cu))]
    bt = i32([[b * 4 + j for j in range(4)] for b in range(3)])
    # mixed: row 0 decodes sequence 0 at position 20, rows 1..5 are the
    # first chunk of sequence 2 (blocks 8..11)
    out.append(model.forward_mixed(
        i32([9, 11, 12, 13, 14, 15]), i32([20, 0, 1, 2, 3, 4]), kv,
        i32([20] + [8 * BS + t for t in range(5)]), 1, bt[:1], i32([21]),
        i32([1]), i32([0]), i32([5]), i32([2]), bt, i32([0, 5]).long()))
    args = (i32([5, 6]), i32([21, 33]), kv, i32([21, 4 * BS + 33]), bt[:2],
            i32([22, 34]))
    out.append(model.forward_decode(*args))
    if graph:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            model.forward_decode(*args)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            logits = model.forward_decode(*args)
        for _ in range(3):
            logits.fill_(NAN)
            gr.replay()
            torch.cuda.synchronize(dev)
            out.append(logits.clone())
    return [o.float().cpu() for o in out]


def _gaps(name, seed=6):
    cfg = get_config(name)
    m = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=seed)
    _set_norms(m, cfg, seed)
    gpu = _steps(m, cfg, DEV, graph=True)
    cpu = _steps(_twin(m, cfg), cfg, "cpu")
    cpu += [cpu[2]] * 3
    return [float((g - c).abs().max() / c.abs().max())
            for g, c in zip(gpu, cpu)]


def test_model_against_cpu_twin():
    """tiny-qk-128 in bf16 on the GPU against forward_* in float32 on the
    CPU with the same weights: prefill, a mixed step, a decode step, and
    the decode step captured and replayed three times.  Each gap is at most
    twice the one the same procedure measures for tiny-128 (the Llama path,
    which runs none of the new code)."""
    base = _gaps("tiny-128")
    got = _gaps("tiny-qk-128")
    names = ["prefill", "mixed", "decode", "graph 1", "graph 2", "graph 3"]
    for n, g, b in zip(names, got, base):
        print(f"{n}: tiny-qk-128 {g:.4e}  tiny-128 {b:.4e}")
    for n, g, b in zip(names, got, base):
        assert g <= 2 * b, (n, g, b)


@pytest.mark.parametrize("mode", ["int4", "fp8kv"])
def test_decode_step_other_modes_finite(mode):
    cfg = get_config("tiny-qk-128")
    m = LlamaForCausalLM(cfg, device=DEV, dtype=BF16, seed=6,
                         quant="int4" if mode == "int4" else None)
    _set_norms(m, cfg, 6)
    kv = PagedKVCache.for_model(cfg, 4, device=DEV,
                                kv_dtype=FP8 if mode == "fp8kv" else BF16)
    i32 = lambda v: _i32(v, DEV)
    n = 20
    m.forward_prefill(i32(list(range(3, 3 + n))), i32(list(range(n))), kv,
                      i32(list(range(n))), i32([0, n]))
    out = m.forward_decode(i32([5]), i32([n]), kv, i32([n]),
                           i32([[0, 1, 2, 3]]), i32([n + 1]))
    assert out.shape == (1, cfg.vocab_size) and out.float().isfinite().all()
    assert kv.k.dtype == (FP8 if mode == "fp8kv" else BF16)


@pytest.mark.parametrize("bad", ["shape", "dtype", "device"])
@pytest.mark.parametrize("op", ["unfused", "fused"])
def test_wrappers_reject_bad_norm_weights(op, bad):
    D, n_q, n_kv = 128, 4, 1
    qkv = torch.zeros(1, (n_q + 2 * n_kv) * D, dtype=BF16, device=DEV)
    w = torch.ones(D, dtype=BF16, device=DEV)
    wrong = {"shape": torch.ones(D // 2, dtype=BF16, device=DEV),
             "dtype": torch.ones(D, device=DEV),
             "device": torch.ones(D, dtype=BF16)}[bad]
    pos = _i32([0], DEV)
    cs = ref.build_cos_sin(8, D).to(DEV)
    kc = torch.zeros(1, n_kv, BS, D, dtype=BF16, device=DEV)
    vc = torch.zeros_like(kc)
    for wq, wk in ((wrong, w), (w, wrong)):
        with pytest.raises(RuntimeError, match="norm_w"):
            if op == "unfused":
                ops.qk_norm_rope_kv_append_qkv_(qkv, wq, wk, EPS, pos, cs, kc,
                                                vc, pos, n_q)
            else:
                ops.decode_attn_qknorm_rope_qkv(
                    qkv, wq, wk, EPS, pos, cs, kc, vc, pos, _i32([[0]], DEV),
                    _i32([1], DEV), D ** -0.5, n_q)
    if op == "fused":       # the fused op serves the engine's block size only
        kc32 = torch.zeros(1, n_kv, 32, D, dtype=BF16, device=DEV)
        with pytest.raises(RuntimeError, match="block_size"):
            ops.decode_attn_qknorm_rope_qkv(
                qkv, w, w, EPS, pos, cs, kc32, kc32.clone(), pos,
                _i32([[0]], DEV), _i32([1], DEV), D ** -0.5, n_q)
