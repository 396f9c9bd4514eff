"""Input constructions, closed-form oracles and the comparator for
tests/test_attn_boundaries.py (a plain helper module, imported the way
tests/gateway_harness.py is).

Three constructions, all over a paged cache with block_size 16:

* RAMP (edge detector).  The key at logical position t is zero except
  k[0] = t // 16 and k[1] = t % 16; every query is zero except
  q[0] = 16c and q[1] = c with c = round(16 * sqrt(D)), so with
  scale = 1/sqrt(D) the score of position t is c*t/sqrt(D) ~= 16*t and
  the softmax is, to ~1e-7, a one-hot on the LAST allowed key.
  V[t][d] = ((7t + 3d) % 17) - 8, so neighbouring positions differ by 10
  in max-norm.  Every number is an integer <= 16 (keys, values) or an
  8-bit-mantissa integer (queries): exact in bf16 and in e4m3, so a bf16
  and an fp8 cache give the same answer.  The ramp continues through
  every slot the kernel must not read; block-table entries past the last
  needed block point at a SPARE in-range block that holds a key larger
  than any valid one (16, 16) and the V code 12, which no position uses.
* UNIFORM (interior detector).  q = 0, so every allowed key weighs
  exactly 1/L; V[t] is the one-hot of channel t % D, so
  out[d] = count/L and one key skipped or counted twice anywhere moves a
  channel by ~1/L.  Tolerance atol = 1/(4L) (a quarter of one key),
  rtol = 2e-2.
* NEEDLE (decode only).  Random K/V; each (sequence, query head) gets
  q = 2 * k_j for its own target position j; successive launches move
  the targets until every j in 0..L-1 has been a needle.

``attend`` is the float64 oracle of the first two: given, per output
row, the set of positions the row may attend to, it returns the exact
softmax-weighted V.  The correct expectation and every deliberately
wrong one (last key dropped, one extra key, an interior key removed,
causal mask shifted) are the same function on a different set.
"""

from __future__ import annotations

import math

import torch

BS = 16                     # cache block size of every case
N_TBL = 17                  # block-table width: 17 blocks = 272 positions
T_MAX = N_TBL * BS - 1      # 271: largest ramp position (digits <= 16)
SPARE = T_MAX + 1           # oracle index of the spare block's rows
SPARE_V = 12.0              # V code no valid position uses
FP8 = torch.float8_e4m3fn
BF16_TOL = 2e-2             # the project's bf16 atol = rtol


# ------------------------------------------------------------ value codes
def ramp_c(D: int) -> int:
    return round(16 * math.sqrt(D))          # 181 (D=128), 128 (D=64)


def ramp_q(D: int) -> torch.Tensor:
    q = torch.zeros(D)
    q[0], q[1] = 16 * ramp_c(D), ramp_c(D)
    return q


def ramp_k(t: torch.Tensor, D: int) -> torch.Tensor:
    """[..., D] keys of logical positions ``t`` (SPARE -> (16, 16))."""
    k = torch.zeros(*t.shape, D)
    sp = t == SPARE
    k[..., 0] = torch.where(sp, torch.tensor(BS), t // BS).float()
    k[..., 1] = torch.where(sp, torch.tensor(BS), t % BS).float()
    return k


def ramp_v(t: torch.Tensor, D: int) -> torch.Tensor:
    d = torch.arange(D)
    v = ((7 * t.unsqueeze(-1) + 3 * d) % 17 - 8).float()
    return torch.where((t == SPARE).unsqueeze(-1), torch.tensor(SPARE_V), v)


def uniform_v(t: torch.Tensor, D: int) -> torch.Tensor:
    v = (torch.arange(D) == (t % D).unsqueeze(-1)).float()
    return torch.where((t == SPARE).unsqueeze(-1), torch.tensor(SPARE_V), v)


def value_table(kind: str, D: int) -> torch.Tensor:
    t = torch.arange(SPARE + 1)
    return ramp_v(t, D) if kind == "ramp" else uniform_v(t, D)


def query_rows(kind: str, rows: int, n_q: int, D: int) -> torch.Tensor:
    """[rows, n_q, D] bf16 queries."""
    q = ramp_q(D) if kind == "ramp" else torch.zeros(D)
    return q.expand(rows, n_q, D).to(torch.bfloat16).contiguous()


def identity_rope(max_pos: int, D: int) -> torch.Tensor:
    """cos = 1, sin = 0 in build_cos_sin's [max_pos, D] layout."""
    return torch.cat([torch.ones(max_pos, D // 2),
                      torch.zeros(max_pos, D // 2)], dim=-1).contiguous()


# ----------------------------------------------------------------- oracle
def attend(kind: str, D: int, allowed: torch.Tensor) -> torch.Tensor:
    """float64 [R, D]: softmax over the allowed positions of each row
    (``allowed`` is bool [R, SPARE + 1]; column SPARE is the spare
    block's code) times V.  A row that may attend to nothing is zero,
    as the kernels' ``den > 0 ? num / den : 0``."""
    assert allowed.shape[1] == SPARE + 1
    t = torch.arange(SPARE + 1)
    if kind == "ramp":
        # the exact score the kernels form: (16c * hi + c * lo) / sqrt(D)
        k = ramp_k(t, D).double()
        s = (k @ ramp_q(D).double()) / math.sqrt(D)
    else:
        s = torch.zeros(SPARE + 1, dtype=torch.float64)
    s = s.expand(allowed.shape[0], -1).masked_fill(~allowed, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return p @ value_table(kind, D).double()


def allowed_upto(n_keys: torch.Tensor) -> torch.Tensor:
    """bool [R, SPARE + 1]: row r may attend to positions < n_keys[r]."""
    return torch.arange(SPARE + 1).unsqueeze(0) < n_keys.unsqueeze(1)


MUTANTS = ("drop_last", "one_extra", "interior_removed")


def mutant(name: str, n_keys: torch.Tensor, limit: torch.Tensor):
    """(allowed, defined) of a deliberately wrong reference.  ``limit``
    is the number of positions that physically exist behind each row
    (272 in a paged cache, the sequence length in a packed prefill
    batch): 'one_extra' exists only where n_keys < limit.  For prefill,
    'drop_last' / 'one_extra' are the causal mask shifted by -1 / +1.

    Named exceptions, the only ones: 'drop_last' of a row with no key
    (seq_len 0) and 'interior_removed' of a row with fewer than two keys
    do not exist — there is nothing to take away.  'drop_last' of a row
    with ONE key does exist here (nothing is left, the output is zero)
    and must be caught."""
    if name == "drop_last":
        return allowed_upto(n_keys - 1), n_keys >= 1
    if name == "one_extra":
        ok = n_keys < limit
        return allowed_upto(torch.where(ok, n_keys + 1, n_keys)), ok
    if name == "interior_removed":
        a = allowed_upto(n_keys)
        ok = n_keys >= 2
        gone = torch.where(ok, (n_keys - 1) // 2, torch.tensor(SPARE))
        a[torch.arange(len(n_keys)), gone] &= ~ok
        return a, ok
    raise ValueError(name)


# what each construction must catch: the ramp sees edges, the uniform
# fill sees everything (one key is worth 1/L there)
CATCHES = {"ramp": ("drop_last", "one_extra"),
           "uniform": MUTANTS}


# ------------------------------------------------------------- comparator
def tolerances(kind: str, n_keys: torch.Tensor):
    """(atol [R, 1], rtol) of a construction: ramp/needle use the
    project's bf16 tolerance; uniform uses a quarter of one key."""
    if kind == "uniform":
        return (1.0 / (4.0 * n_keys.clamp_min(1).double())).unsqueeze(1), 2e-2
    return torch.full((len(n_keys), 1), BF16_TOL, dtype=torch.float64), BF16_TOL


def bad_rows(got: torch.Tensor, want: torch.Tensor, atol, rtol: float):
    """bool [R]: rows of ``got`` [R, ...] outside atol + rtol*|want|
    (``atol`` a float or per-row [R, 1]).  THE comparator: the GPU tests
    and the CPU power checks both go through it."""
    g = got.double().reshape(got.shape[0], -1)
    w = want.double().reshape(want.shape[0], -1)
    err = (g - w).abs()
    ok = err <= atol + rtol * w.abs()
    return ~(ok & torch.isfinite(g)).all(dim=1)


# ------------------------------------------------------------ paged cache
def paged_cache(kind: str, n_seqs: int, n_kv: int, D: int,
                dtype=torch.bfloat16, seed: int = 0):
    """(k_cache, v_cache, table [n_seqs, 17], spare) — every sequence
    owns 17 permuted physical blocks holding logical positions 0..271 of
    the construction (so the ramp runs on past any seq_len); block
    ``spare`` is the poison block.  Use ``block_table`` for the per-launch
    table, which redirects unneeded entries to the spare."""
    g = torch.Generator().manual_seed(seed)
    n_phys = n_seqs * N_TBL + 1
    perm = torch.randperm(n_phys, generator=g)
    spare = int(perm[-1])
    table = perm[:-1].reshape(n_seqs, N_TBL).to(torch.int32)
    t = torch.arange(N_TBL * BS).reshape(N_TBL, 1, BS)
    klog = ramp_k(t, D)                               # [17, 1, 16, D]
    vlog = ramp_v(t, D) if kind == "ramp" else uniform_v(t, D)
    kc = torch.empty(n_phys, n_kv, BS, D)
    vc = torch.empty(n_phys, n_kv, BS, D)
    flat = table.long().reshape(-1)
    kc[flat] = klog.repeat(n_seqs, 1, 1, 1).expand(-1, n_kv, -1, -1)
    vc[flat] = vlog.repeat(n_seqs, 1, 1, 1).expand(-1, n_kv, -1, -1)
    sp = torch.full((BS,), SPARE)
    kc[spare] = ramp_k(sp, D)
    vc[spare] = SPARE_V
    return kc.to(dtype), vc.to(dtype), table, spare


def block_table(table: torch.Tensor, n_keys, spare: int) -> torch.Tensor:
    """Per-launch table: entries past the last block that ``n_keys[i]``
    positions need are redirected to the spare block."""
    need = (torch.as_tensor(n_keys) + BS - 1) // BS
    j = torch.arange(table.shape[1]).unsqueeze(0)
    return torch.where(j < need.unsqueeze(1), table,
                       torch.tensor(spare, dtype=torch.int32)).contiguous()


# ------------------------------------------------------------ decode cases
# (batch, n_q, n_kv, D, split factor the ops must pick)
DECODE_SHAPES = [
    (48, 32, 8, 128, 1),
    (32, 32, 8, 128, 2),
    (24, 16, 8, 128, 3),
    (4, 8, 2, 64, 16),
    (48, 8, 8, 64, 1),
]

_MULT16 = list(range(16, 257, 16))
# 0 first (must return zeros), the lengths the cases must include, then
# both sides of every multiple of 16 and the multiples themselves
DECODE_LENS = list(dict.fromkeys(
    [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256,
     257, 271]
    + [m + s for m in _MULT16 for s in (-1, 1)] + _MULT16))


def decode_launches(batch: int, fused: bool = False):
    """DECODE_LENS cut into launches of ``batch`` rows (the last launch
    wraps round to stay full, so the split factor is the case's own).
    The fused op appends one token, so it has no seq_len 0 row."""
    lens = [l for l in DECODE_LENS if l > 0 or not fused]
    out = []
    for i in range(0, len(lens), batch):
        chunk = lens[i:i + batch]
        chunk += lens[:batch - len(chunk)]
        out.append(torch.tensor(chunk))
    return out


def needle_len(n_split: int) -> int:
    """Shortest L (+8 so the tail block is partial) at which each of the
    4 * n_split wave chains walks at least three blocks."""
    return 3 * 4 * n_split * BS + 8


def needle_case(batch, n_q, n_kv, D, n_split, dtype=torch.bfloat16, seed=0):
    """Random cache of ``batch`` sequences of length needle_len(n_split)
    and the target rounds: in round r, (sequence i, head h) looks for
    position rounds[r][i, h].  One launch holds batch * n_q needles, so
    the rounds together make EVERY position 0..L-1 a needle once (the
    last round wraps round to stay full).  Returns
    (k_cache, v_cache, block_table, seq_lens, rounds)."""
    g = torch.Generator().manual_seed(seed)
    L = needle_len(n_split)
    nb = (L + BS - 1) // BS
    n_phys = batch * nb + 1
    kc = torch.randn(n_phys, n_kv, BS, D, generator=g).to(dtype)
    vc = torch.randn(n_phys, n_kv, BS, D, generator=g).to(dtype)
    bt = torch.randperm(n_phys, generator=g)[:batch * nb] \
        .reshape(batch, nb).to(torch.int32).contiguous()
    pairs = batch * n_q
    rounds = [((r + torch.arange(pairs)) % L).reshape(batch, n_q)
              for r in range(0, L, pairs)]
    lens = torch.full((batch,), L, dtype=torch.int32)
    return kc, vc, bt, lens, rounds


def needle_queries(kc, bt, targets):
    """[batch, n_q, D] bf16: q[i, h] = 2 * k at position targets[i, h] of
    sequence i, in the kv head that query head h reads."""
    batch, n_q = targets.shape
    group = n_q // kc.shape[1]
    phys = bt.long().gather(1, targets // BS)                  # [B, n_q]
    kvh = (torch.arange(n_q) // group).expand(batch, n_q)
    q = 2 * kc.float()[phys, kvh, targets % BS]
    return q.to(torch.bfloat16).contiguous()


def decode_oracle(q, kc, vc, bt, lens, scale, drop=None):
    """float64 paged decode attention, batched; ``drop`` [batch, n_q]
    removes one logical position per (sequence, head) (-1: none)."""
    B, n_q, D = q.shape
    n_kv = kc.shape[1]
    g = n_q // n_kv
    nb = max((int(lens.max()) + BS - 1) // BS, 1)
    blocks = bt[:, :nb].long()
    K = kc.float()[blocks].permute(0, 2, 1, 3, 4).reshape(B, n_kv, nb * BS, D)
    V = vc.float()[blocks].permute(0, 2, 1, 3, 4).reshape(B, n_kv, nb * BS, D)
    s = torch.einsum("bhgd,bhtd->bhgt", q.double().view(B, n_kv, g, D),
                     K.double()) * scale
    t = torch.arange(nb * BS)
    mask = (t >= lens.long().view(B, 1, 1, 1)).expand_as(s)
    if drop is not None:
        mask = mask | (t == drop.view(B, n_kv, g, 1))
    p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
    o = torch.einsum("bhgt,bhtd->bhgd", torch.nan_to_num(p, nan=0.0),
                     V.double())
    return o.reshape(B, n_q, D)


# ----------------------------------------------------------- prefill cases
PREFILL_LENS = [1, 31, 32, 33, 63, 64, 65, 129, 271]
# (n_q, n_kv, D): groups 4, 1, 2, 8 and D = 64 once
PREFILL_SHAPES = [(32, 8, 128), (8, 8, 128), (16, 8, 128), (16, 2, 128),
                  (8, 2, 64)]


def prefill_positions(lens=PREFILL_LENS):
    """(pos [T], seq_len_of_row [T], cu_seqlens [n+1] int32)."""
    pos = torch.cat([torch.arange(l) for l in lens])
    own = torch.cat([torch.full((l,), l) for l in lens])
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)),
                      dtype=torch.int32)
    return pos, own, cu


def prefill_qkv(kind: str, n_q: int, n_kv: int, D: int, lens=PREFILL_LENS):
    """Packed [T, (n_q + 2 n_kv) D] bf16 batch: row at position t of its
    sequence carries the construction's q, k(t), v(t).  The previous
    sequence's last rows carry its HIGHEST keys — backward poison."""
    pos, _, _ = prefill_positions(lens)
    T = len(pos)
    q = query_rows(kind, T, n_q, D).float()
    k = ramp_k(pos, D).unsqueeze(1).expand(T, n_kv, D)
    v = (ramp_v(pos, D) if kind == "ramp" else uniform_v(pos, D)) \
        .unsqueeze(1).expand(T, n_kv, D)
    return torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)],
                     dim=1).to(torch.bfloat16).contiguous()


def prefill_as_paged(qkv, n_q: int, n_kv: int, D: int, lens=PREFILL_LENS,
                     seed: int = 0):
    """The packed bf16 batch ``qkv`` restated for the paged entry: a bf16
    cache that holds each sequence's own K/V behind a shuffled block
    table (one table row per sequence; every other slot holds the spare
    code), and each sequence cut into chunks of <= 32 rows (row0 = t,
    pos0 = t - cu[s], btrow = s).  Returns (k_cache, v_cache,
    block_table, chunks) with ``chunks`` a dict of int32 tensors."""
    pos, _, cu = prefill_positions(lens)
    T, n = len(pos), len(lens)
    g = torch.Generator().manual_seed(seed)
    n_phys = n * N_TBL + 1
    bt = torch.randperm(n_phys, generator=g)[:-1] \
        .reshape(n, N_TBL).to(torch.int32).contiguous()
    seq = torch.repeat_interleave(torch.arange(n), torch.tensor(lens))
    phys = bt.long()[seq, pos // BS]
    kc = torch.full((n_phys, n_kv, BS, D), SPARE_V, dtype=torch.bfloat16)
    vc = kc.clone()
    kc[phys, :, pos % BS] = qkv[:, n_q * D:(n_q + n_kv) * D].reshape(T, n_kv, D)
    vc[phys, :, pos % BS] = qkv[:, (n_q + n_kv) * D:].reshape(T, n_kv, D)
    cu = cu.tolist()
    rows = [(t, t - cu[s], min(32, cu[s + 1] - t), s)
            for s in range(n) for t in range(cu[s], cu[s + 1], 32)]
    chunks = {name: torch.tensor([r[i] for r in rows], dtype=torch.int32)
              for i, name in enumerate(("row0", "pos0", "nrows", "btrow"))}
    return kc, vc, bt, chunks


# ----------------------------------------------------- paged-prefill cases
# (block-table row, pos0, nrows); engine-style <= 32-row kernel chunks
PAGED_CHUNKS = [
    (0, 183, 17), (0, 200, 32),          # one sequence, four 64-wide KV tiles
    (1, 63, 1), (1, 64, 1), (1, 128, 1), (1, 270, 1),   # decode-like rows
    (2, 0, 32), (2, 32, 8),              # a fresh sequence
    (3, 17, 5),                          # starts mid cache block
]
PAGED_SHAPES = [(32, 8, 128), (16, 2, 128), (8, 8, 128), (8, 2, 64)]
PAGED_PAD = 3        # rows no chunk covers, after every chunk's rows


def paged_chunks():
    """Chunk tensors + per-covered-row metadata.  Rows the chunks do not
    cover (PAGED_PAD after each chunk) stay uncompared: the op's output
    is ``empty`` there."""
    row0s, rows, pos, btrow_of_row = [], [], [], []
    r = 0
    for btr, p0, n in PAGED_CHUNKS:
        row0s.append(r)
        rows += list(range(r, r + n))
        pos += list(range(p0, p0 + n))
        btrow_of_row += [btr] * n
        r += n + PAGED_PAD
    n_rows = len({c[0] for c in PAGED_CHUNKS})
    kv_hi = [max(p0 + n for b, p0, n in PAGED_CHUNKS if b == i)
             for i in range(n_rows)]
    i32 = dict(dtype=torch.int32)
    return dict(
        T=r,
        row0=torch.tensor(row0s, **i32),
        pos0=torch.tensor([c[1] for c in PAGED_CHUNKS], **i32),
        nrows=torch.tensor([c[2] for c in PAGED_CHUNKS], **i32),
        btrow=torch.tensor([c[0] for c in PAGED_CHUNKS], **i32),
        rows=torch.tensor(rows), pos=torch.tensor(pos),
        kv_hi=torch.tensor(kv_hi), n_tables=n_rows)


def paged_qkv(kind: str, T: int, n_q: int, n_kv: int, D: int):
    """[T, (n_q + 2 n_kv) D]: construction queries; the k/v columns (the
    op reads K/V from the cache, never from here) hold the spare code."""
    q = query_rows(kind, T, n_q, D).float().reshape(T, -1)
    kv = torch.full((T, 2 * n_kv * D), SPARE_V)
    return torch.cat([q, kv], dim=1).to(torch.bfloat16).contiguous()
