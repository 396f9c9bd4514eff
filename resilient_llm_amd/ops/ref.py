"""Pure-PyTorch fp32 reference implementations of every HIP op.

These are (a) the ground truth the GPU numerics tests compare the gfx950
kernels against (SURVEY.md §4 implication (b)) and (b) the CPU execution
path for the plumbing tests — the model runs end-to-end on CPU through
these exact functions.  Semantics match the kernels bit-for-bit where the
kernels round (bf16 storage boundaries), computed in fp32.
"""

from __future__ import annotations

import torch


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def rmsnorm_residual_(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                      eps: float) -> torch.Tensor:
    """residual += x (stored at residual dtype); y = rmsnorm(residual)."""
    summed = (x.float() + residual.float()).to(residual.dtype)
    residual.copy_(summed)
    return rmsnorm(residual, w, eps)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    inter = gate_up.shape[-1] // 2
    g = gate_up[..., :inter].float()
    u = gate_up[..., inter:].float()
    return (torch.nn.functional.silu(g) * u).to(gate_up.dtype)


def build_cos_sin(max_pos: int, head_dim: int, theta: float = 500000.0,
                  device="cpu") -> torch.Tensor:
    """[max_pos, head_dim] f32: row = [cos(0..D/2) | sin(0..D/2)]."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half, dtype=torch.float64) / half))
    pos = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(pos, inv_freq)
    return torch.cat([ang.cos(), ang.sin()], dim=-1).float().to(device)


def _rotate(x: torch.Tensor, positions: torch.Tensor,
            cos_sin: torch.Tensor) -> torch.Tensor:
    """GPT-NeoX half rotation; x [T, H, D]."""
    D = x.shape[-1]
    half = D // 2
    cs = cos_sin[positions.long()]                  # [T, D]
    cos = cs[:, :half].unsqueeze(1)                 # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1)
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    out = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    return out.to(x.dtype)


def rope_kv_append_(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    positions: torch.Tensor, cos_sin: torch.Tensor,
                    k_cache: torch.Tensor, v_cache: torch.Tensor,
                    slot_mapping: torch.Tensor) -> None:
    q.copy_(_rotate(q, positions, cos_sin))
    k.copy_(_rotate(k, positions, cos_sin))
    block_size = k_cache.shape[2]
    slots = slot_mapping.long()
    valid = slots >= 0
    idx = slots[valid]
    blocks = idx // block_size
    rows = idx % block_size
    # cache: [num_blocks, n_kv, block_size, D]; k/v: [T, n_kv, D]
    # cast through the cache dtype (bf16 identity; fp8-e4m3 quantizes —
    # mirrors the GPU codec's cvt_pk_fp8 RNE conversion)
    k_cache[blocks, :, rows] = k[valid].to(k_cache.dtype)
    v_cache[blocks, :, rows] = v[valid].to(v_cache.dtype)


def decode_attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                block_table: torch.Tensor, seq_lens: torch.Tensor,
                scale: float) -> torch.Tensor:
    batch, n_q, D = q.shape
    n_kv = k_cache.shape[1]
    block_size = k_cache.shape[2]
    group = n_q // n_kv
    out = torch.empty_like(q)
    for b in range(batch):
        L = int(seq_lens[b])
        n_blocks = (L + block_size - 1) // block_size
        blocks = block_table[b, :n_blocks].long()
        k = k_cache[blocks].transpose(0, 1).reshape(n_kv, -1, D)[:, :L].float()
        v = v_cache[blocks].transpose(0, 1).reshape(n_kv, -1, D)[:, :L].float()
        qb = q[b].float().view(n_kv, group, D)
        s = torch.einsum("hgd,htd->hgt", qb, k) * scale
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgt,htd->hgd", p, v)
        out[b] = o.reshape(n_q, D).to(q.dtype)
    return out


def prefill_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 cu_seqlens: torch.Tensor, scale: float) -> torch.Tensor:
    T, n_q, D = q.shape
    n_kv = k.shape[1]
    group = n_q // n_kv
    out = torch.empty_like(q)
    cu = cu_seqlens.tolist()
    for s in range(len(cu) - 1):
        s0, s1 = cu[s], cu[s + 1]
        L = s1 - s0
        qs = q[s0:s1].float().view(L, n_kv, group, D)
        ks = k[s0:s1].float()
        vs = v[s0:s1].float()
        scores = torch.einsum("qhgd,thd->hgqt", qs, ks) * scale
        mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=q.device), 1)
        scores.masked_fill_(mask, float("-inf"))
        p = torch.softmax(scores, dim=-1)
        o = torch.einsum("hgqt,thd->qhgd", p, vs)
        out[s0:s1] = o.reshape(L, n_q, D).to(q.dtype)
    return out


def prefill_paged_attn(qkv: torch.Tensor, k_cache: torch.Tensor,
                       v_cache: torch.Tensor, chunk_row0, chunk_pos0,
                       chunk_nrows, chunk_btrow, block_tables,
                       scale: float, n_q: int) -> torch.Tensor:
    """Chunked prefill over the paged cache: each chunk's q rows attend
    causally over their sequence's cached prefix (which includes the
    chunk itself — rope_kv_append ran first)."""
    T = qkv.shape[0]
    n_kv, block_size, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    group = n_q // n_kv
    out = torch.zeros(T, n_q * D, dtype=qkv.dtype)
    for c in range(len(chunk_row0)):
        row0 = int(chunk_row0[c]); pos0 = int(chunk_pos0[c])
        nrows = int(chunk_nrows[c]); btr = int(chunk_btrow[c])
        kv_hi = pos0 + nrows
        n_blocks = (kv_hi + block_size - 1) // block_size
        blocks = block_tables[btr, :n_blocks].long()
        k = k_cache[blocks].transpose(0, 1).reshape(n_kv, -1, D)[:, :kv_hi].float()
        v = v_cache[blocks].transpose(0, 1).reshape(n_kv, -1, D)[:, :kv_hi].float()
        q = qkv[row0:row0 + nrows, :n_q * D].reshape(nrows, n_kv, group, D).float()
        s = torch.einsum("qhgd,htd->hgqt", q, k) * scale
        qpos = torch.arange(pos0, pos0 + nrows).unsqueeze(1)
        kvpos = torch.arange(kv_hi).unsqueeze(0)
        s.masked_fill_((kvpos > qpos), float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgqt,htd->qhgd", p, v)
        out[row0:row0 + nrows] = o.reshape(nrows, n_q * D).to(qkv.dtype)
    return out


def sample(logits: torch.Tensor, temperatures: torch.Tensor,
           seeds: torch.Tensor, step: int = 0) -> torch.Tensor:
    """Greedy rows match the kernel exactly; stochastic rows use torch
    RNG seeded per row from (seeds[i], step) — same reproducibility
    contract as the kernel, not bitwise the same stream."""
    out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    lf = logits.float()
    greedy = temperatures <= 0
    if greedy.any():
        out[greedy] = lf[greedy].argmax(-1).to(torch.int32)
    C = 0x9e3779b97f4a7c15
    for i in (~greedy).nonzero(as_tuple=True)[0].tolist():
        gen = torch.Generator(device=logits.device)
        gen.manual_seed((int(seeds[i]) + C * step) & 0x7fffffffffffffff)
        probs = torch.softmax(lf[i] / float(temperatures[i]), dim=-1)
        out[i] = int(torch.multinomial(probs, 1, generator=gen))
    return out


def sample_constrained(logits: torch.Tensor, rows: torch.Tensor,
                       temperatures: torch.Tensor, seeds: torch.Tensor,
                       step: int, top_k: torch.Tensor, min_p: torch.Tensor,
                       bias_offsets: torch.Tensor, bias_ids: torch.Tensor,
                       bias_vals: torch.Tensor) -> torch.Tensor:
    """``sample`` under logit_bias / top_k / min_p for the selected rows.
    z = float(logit) + bias in fp32; kept = {z >= k-th largest z} (ties
    stay; k == 0 or k >= vocab off) & {z >= z_max + T*ln(min_p)} (0 off).
    Greedy rows are exact (arg-max z, lowest index); stochastic rows draw
    from softmax(z/T) renormalised over the kept set with a torch
    generator seeded per row from (seeds[rows[r]], step) — the kernel's
    reproducibility contract, not its stream."""
    R = rows.numel()
    if not (top_k.numel() == R and min_p.numel() == R
            and bias_offsets.numel() == R + 1):
        raise ValueError("rows/top_k/min_p/bias_offsets length mismatch")
    if bias_ids.numel() != bias_vals.numel():
        raise ValueError("bias_ids/bias_vals length mismatch")
    V = logits.shape[1]
    out = torch.empty(R, dtype=torch.int32, device=logits.device)
    offs = bias_offsets.tolist()
    C = 0x9e3779b97f4a7c15
    for r, row in enumerate(rows.tolist()):
        z = logits[row].float()
        b0, b1 = offs[r], offs[r + 1]
        if b1 > b0:
            z = z.clone()
            z[bias_ids[b0:b1].long()] += bias_vals[b0:b1].float()
        T = float(temperatures[row])
        if T <= 0:
            out[r] = int(z.argmax())
            continue
        keep = torch.ones(V, dtype=torch.bool, device=z.device)
        k = int(top_k[r])
        if 1 <= k < V:
            keep &= z >= z.topk(k).values[-1]
        m = float(min_p[r])
        if m > 0:
            keep &= z >= z.max() + torch.tensor(T, dtype=torch.float32) \
                * torch.log(torch.tensor(m, dtype=torch.float32))
        probs = torch.softmax(
            torch.where(keep, z, z.new_tensor(float("-inf"))) / T, dim=-1)
        gen = torch.Generator(device=logits.device)
        gen.manual_seed((int(seeds[row]) + C * step) & 0x7fffffffffffffff)
        out[r] = int(torch.multinomial(probs, 1, generator=gen))
    return out


def token_logprobs(logits: torch.Tensor, rows: torch.Tensor,
                   tokens: torch.Tensor, k: int):
    """Log-softmax (fp32, RAW logits — independent of temperature, top-p
    and penalties) of ``tokens[i]`` in row ``rows[i]``, plus that row's
    ``k`` most likely tokens ordered by value descending, index ascending
    on ties.  Returns (chosen_lp [R] f32, top_lp [R, k] f32,
    top_ids [R, k] int32)."""
    if not 0 <= k <= min(20, logits.shape[1]):
        raise ValueError(f"k must be in [0, min(20, vocab)], got {k}")
    if rows.numel() != tokens.numel():
        raise ValueError("rows/tokens length mismatch")
    ridx = rows.long()
    lp = torch.log_softmax(logits.index_select(0, ridx).float(), dim=-1)
    chosen = lp.gather(1, tokens.long().unsqueeze(1)).squeeze(1)
    vals, ids = torch.sort(lp, dim=-1, descending=True, stable=True)
    return chosen, vals[:, :k].contiguous(), ids[:, :k].to(torch.int32)


def kv_copy_blocks_(k_cache: torch.Tensor, v_cache: torch.Tensor,
                    src: torch.Tensor, dst: torch.Tensor) -> None:
    """In place, bit-exact: cache[l, dst[p]] = cache[l, src[p]] for every
    layer l and pair p, for both [L, NB, H, bs, D] caches.  Works on the
    raw bytes, so any element type (bf16, fp8, fp32) copies alike.  ``src``
    may repeat; ``dst`` entries are unique and disjoint from ``src``."""
    if src.numel() != dst.numel():
        raise ValueError("src/dst length mismatch")
    if src.numel() == 0:
        return
    s, d = src.long(), dst.long()
    for cache in (k_cache, v_cache):
        if cache.dim() != 5 or not cache.is_contiguous():
            raise ValueError("cache must be contiguous [L, NB, H, bs, D]")
        raw = cache.view(torch.uint8)
        raw[:, d] = raw[:, s]


# ---- batched multi-adapter LoRA ----
# The rounding contract of the HIP kernels (ops/csrc/lora.hip): the shrink
# result y and the delta stay in f32; there is ONE rounding, to out's
# dtype, at the final add.  Token row t uses adapter adapter_idx[t]; -1
# (or an index outside the stack) means no adapter.
def _adapter_rows(adapter_idx: torch.Tensor, n_adapters: int):
    idx = adapter_idx.long()
    for a in torch.unique(idx).tolist():
        if 0 <= a < n_adapters:
            yield a, (idx == a).nonzero().squeeze(1)


def lora_shrink(x: torch.Tensor, A: torch.Tensor,
                adapter_idx: torch.Tensor) -> torch.Tensor:
    """y[t, r] = sum_k x[t, k] * A[a(t), r, k] in f32: x [T, K],
    A [n_adapters, R, K], adapter_idx [T] int32 -> y [T, R] f32.  Rows
    without an adapter are zero here (the device op leaves them
    unwritten; nothing reads them)."""
    y = torch.zeros((x.shape[0], A.shape[1]), dtype=torch.float32,
                    device=x.device)
    for a, rows in _adapter_rows(adapter_idx, A.shape[0]):
        y[rows] = x[rows].float() @ A[a].float().t()
    return y


def lora_expand_add_(out: torch.Tensor, y: torch.Tensor, B: torch.Tensor,
                     scale: torch.Tensor, slices,
                     adapter_idx: torch.Tensor) -> torch.Tensor:
    """In place: out[t, o] = dtype(float(out[t, o]) + scale[a] * sum_j
    y[t, s*r_max + j] * B[a, o, j]) with s the slice of output row o under
    the ascending end-exclusive boundaries ``slices`` (<= 3, the last one
    == O): out [T, O], y [T, len(slices) * r_max] f32,
    B [n_adapters, O, r_max], scale [n_adapters] f32.  Rows without an
    adapter are not touched."""
    slices = [int(e) for e in slices]
    O, r_max = B.shape[1], B.shape[2]
    if not 1 <= len(slices) <= 3 or slices != sorted(set(slices)) \
            or slices[0] <= 0 or slices[-1] != O or out.shape[1] != O:
        raise ValueError(f"bad slice table {slices} for O = {O}")
    if y.shape[1] != len(slices) * r_max:
        raise ValueError("y width must be len(slices) * r_max")
    for a, rows in _adapter_rows(adapter_idx, B.shape[0]):
        yr = y[rows]
        delta = torch.empty((rows.numel(), O), dtype=torch.float32,
                            device=out.device)
        lo = 0
        for s, hi in enumerate(slices):
            delta[:, lo:hi] = (yr[:, s * r_max:(s + 1) * r_max]
                               @ B[a, lo:hi].float().t())
            lo = hi
        out[rows] = (out[rows].float()
                     + scale[a].float() * delta).to(out.dtype)
    return out


# ---- fp8-activation emitters (quantized-weight GEMM path) ----
def quantize_fp8_rowwise(t: torch.Tensor):
    """Per-row fp8-e4m3 quantization: (q, scales) with q*scales ~= t."""
    f = t.float()
    amax = f.abs().amax(dim=-1).clamp_min(1e-12)
    scales = amax / 448.0
    q = (f / scales.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q, scales


def rmsnorm_fp8(x, w, eps=1e-5):
    return quantize_fp8_rowwise(rmsnorm(x, w, eps))


def rmsnorm_residual_fp8(x, residual, w, eps=1e-5):
    return quantize_fp8_rowwise(rmsnorm_residual_(x, residual, w, eps))


def silu_mul_fp8(gate_up):
    return quantize_fp8_rowwise(silu_mul(gate_up))


def scaled_mm_ref(x8, xs, w8, ws):
    """Dequantized reference of a rowwise torch._scaled_mm: x8 [M,K] fp8
    with per-row scales xs [M], w8 [N,K] fp8 with per-row (out-channel)
    scales ws [N]; bf16 result.  The CPU engine path uses this (no
    hipBLASLt fp8 GEMM off-GPU)."""
    xf = x8.float() * xs.reshape(-1, 1)
    wf = w8.float() * ws.reshape(-1, 1)
    return (xf @ wf.t()).to(torch.bfloat16)


# ---- int4 group-quantized weights (W4A16) ----
# Symmetric, group-wise along K (group = 128): s[n, g] = bf16(max|W| / 7),
# q = clamp(rne(W / s), -8, 7).  ``packed`` is an opaque int32 tensor of
# N*K/8 elements in MFMA fragment order (mfma_f32_16x16x32_bf16): the
# four dwords at ((tile * G + g) * 64 + lane) * 4, tile = n // 16,
# lane = o * 16 + n % 16, hold lane's k-octet o of the four 32-k granules
# of group g — one 16-byte load per lane feeds 4 MFMAs and ends on a scale
# boundary, and a wave's load of one (tile, group) is 1 KiB contiguous.
# Dword j holds k = g*128 + j*32 + o*8 + i, i = 0..7, as the nibble
# u = q + 8 at bit 4*(i//2) + 16*(i%2): ``(d >> 4p) & 0x000F000F |
# 0x43004300`` is then the bf16 pair (128 + u) of elements 2p, 2p+1.
W4_GROUP = 128
_W4_SHIFTS = (0, 16, 4, 20, 8, 24, 12, 28)


def _w4_check_shape(N: int, K: int) -> None:
    if N <= 0 or K <= 0 or N % 64 or K % W4_GROUP:
        raise ValueError(f"int4 weights need N % 64 == 0 and K % 128 == 0, "
                         f"got N={N} K={K}")


def quantize_w4(w: torch.Tensor):
    """W [N, K] -> (q int8 [N, K] in -8..7, s bf16 [N, K/128]).  An
    all-zero group gets the smallest positive normal bf16 as its scale."""
    N, K = w.shape
    _w4_check_shape(N, K)
    f = w.float().reshape(N, K // W4_GROUP, W4_GROUP)
    tiny = torch.finfo(torch.bfloat16).tiny
    s = (f.abs().amax(dim=-1) / 7.0).to(torch.bfloat16)
    s = torch.where(s.float() < tiny, torch.full_like(s, tiny), s)
    q = torch.round(f / s.float().unsqueeze(-1)).clamp_(-8, 7)
    return q.reshape(N, K).to(torch.int8), s.contiguous()


def w4_pack(q: torch.Tensor) -> torch.Tensor:
    """q int8 [N, K] in -8..7 -> opaque int32 [N*K/8] (layout above)."""
    N, K = q.shape
    _w4_check_shape(N, K)
    G = K // W4_GROUP
    u = (q.to(torch.int64) + 8)
    if int(u.min()) < 0 or int(u.max()) > 15:
        raise ValueError("w4_pack: q must be in -8..7")
    # [tile, c, g, j, o, i] -> [tile, g, o, c, j, i]
    u = u.reshape(N // 16, 16, G, 4, 4, 8).permute(0, 2, 4, 1, 3, 5)
    shifts = torch.tensor(_W4_SHIFTS, dtype=torch.int64, device=q.device)
    d = (u << shifts).sum(dim=-1)                  # 0 .. 2^32 - 1
    d = torch.where(d >= 2 ** 31, d - 2 ** 32, d)  # two's-complement int32
    return d.to(torch.int32).reshape(-1).contiguous()


def w4_unpack(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of ``w4_pack``: int8 [N, K] in -8..7."""
    _w4_check_shape(N, K)
    if packed.dtype != torch.int32 or packed.numel() != N * K // 8:
        raise ValueError(f"packed must be int32 with N*K/8 = {N * K // 8} "
                         f"elements, got {packed.dtype} x {packed.numel()}")
    G = K // W4_GROUP
    d = packed.to(torch.int64).reshape(N // 16, G, 4, 16, 4, 1)
    shifts = torch.tensor(_W4_SHIFTS, dtype=torch.int64, device=packed.device)
    u = (d >> shifts) & 15                         # [tile, g, o, c, j, i]
    q = (u - 8).permute(0, 3, 1, 4, 2, 5)          # [tile, c, g, j, o, i]
    return q.reshape(N, K).to(torch.int8).contiguous()


def _w4_shape(packed: torch.Tensor, s: torch.Tensor):
    N, G = s.shape
    return N, G * W4_GROUP


def w4a16_linear(x: torch.Tensor, packed: torch.Tensor,
                 s: torch.Tensor) -> torch.Tensor:
    """The semantic contract of the fused op: out[m, n] = round(sum_g
    f32(s[n, g]) * sum_{k in g} f32(x[m, k]) * q[n, k]) — integer weights
    enter the products unrounded, the scale multiplies each group's
    partial sum, one rounding at the end (to x's dtype: bf16 in, bf16
    out)."""
    N, K = _w4_shape(packed, s)
    G = K // W4_GROUP
    q = w4_unpack(packed, N, K).float().reshape(N, G, W4_GROUP)
    xf = x.float().reshape(x.shape[0], G, W4_GROUP)
    part = torch.einsum("mgk,ngk->mng", xf, q)
    return (part * s.float().unsqueeze(0)).sum(dim=-1).to(x.dtype)


def w4_dequant(packed: torch.Tensor, s: torch.Tensor,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 [N, K] = bf16(f32(s) * q): one rounding per weight."""
    N, K = _w4_shape(packed, s)
    q = w4_unpack(packed, N, K).float().reshape(N, K // W4_GROUP, W4_GROUP)
    w = (q * s.float().unsqueeze(-1)).reshape(N, K).to(torch.bfloat16)
    if out is None:
        return w
    out.copy_(w)
    return out
