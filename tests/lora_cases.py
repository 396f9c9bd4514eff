"""Shared inputs for the LoRA tests: the kernel grid of the exact-integer
and random-data cases (CPU tensors from seeded generators, so the CPU
check of the reference's own order sensitivity and the device tests see
the same data), and PEFT-named random adapters for the engine tests."""

import itertools

import torch

from resilient_llm_amd.ops import ref

BF16 = torch.bfloat16

T_VALUES = (1, 3, 65, 257)
K_VALUES = (8, 256, 520, 4096)
O_VALUES = (8, 264, 6144)
R_MAX_VALUES = (1, 8, 16, 64)
N_SLICES_VALUES = (1, 2, 3)
# end-exclusive slice boundaries per (O, n_slices); none but the last is
# a multiple of 64 and the slice widths are unequal
SLICES = {
    (8, 1): [8], (8, 2): [3, 8], (8, 3): [3, 5, 8],
    (264, 1): [264], (264, 2): [130, 264], (264, 3): [70, 130, 264],
    (6144, 1): [6144], (6144, 2): [4100, 6144], (6144, 3): [4100, 5130, 6144],
}
N_ADAPTERS = 3
IDX_CYCLE = (2, -1, 0, 1)     # -1 rows interleave; the last adapter is used
SCALES = (0.5, 2.0, 0.25)     # powers of two

# (r_max, n_slices) is the parametrised axis; each case walks every
# (T, K, O) of the grid
RANK_CASES = list(itertools.product(R_MAX_VALUES, N_SLICES_VALUES))
SHAPES = list(itertools.product(T_VALUES, K_VALUES, O_VALUES))


def adapter_idx_of(T):
    return torch.tensor([IDX_CYCLE[t % 4] for t in range(T)],
                        dtype=torch.int32)


def run_idx_of(T):
    """Runs of 6 rows per adapter (-1, 0, 1, 2, -1, ...): against the
    kernels' 4-token tiles this gives tiles that share one adapter, tiles
    that mix two, and tiles with and without -1 rows."""
    return torch.tensor([(t // 6) % 4 - 1 for t in range(T)],
                        dtype=torch.int32)


def _seed(kind, T, K, O, r_max, n_slices):
    seed = kind
    for v in (T, K, O, r_max, n_slices):
        seed = (seed * 8209 + v) % 0x7fffffff
    return seed


def integer_case(T, K, O, r_max, n_slices):
    """x, A, B in {-2..2}, out in {-8..8}: with the power-of-two scales
    every partial sum is an exactly representable f32 in any order
    (|y| <= 4K <= 2^14, |sum_j| <= 2^14 * 2 * 64 = 2^21, the scaled delta
    plus out stays below 2^23 in steps of 1/4), so kernel and reference
    round the SAME f32 value to bf16: bit equality."""
    g = torch.Generator().manual_seed(_seed(0, T, K, O, r_max, n_slices))
    R = n_slices * r_max

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g).to(BF16)
    return dict(x=ints((T, K), -2, 2), A=ints((N_ADAPTERS, R, K), -2, 2),
                B=ints((N_ADAPTERS, O, r_max), -2, 2),
                out=ints((T, O), -8, 8),
                scale=torch.tensor(SCALES, dtype=torch.float32),
                slices=SLICES[(O, n_slices)], idx=adapter_idx_of(T))


def random_case(T, K, O, r_max, n_slices):
    """Random bf16 data for the 1-ulp comparison.  Two f32 evaluations
    that differ only in summation order differ by a few f32 ulps of the
    LARGEST term, so they land within one bf16 ulp of each other only
    where the result does not cancel: |out| is drawn from [0.5, 2) and the
    delta (x ~ N(0,1), A ~ N(0,1)/sqrt(K), B ~ N(0,1)/(50 sqrt(r_max)),
    scale <= 2) has a standard deviation <= 0.04 beside it, so cancelling
    an |out| >= 0.5 would take a 12-sigma delta."""
    g = torch.Generator().manual_seed(_seed(1, T, K, O, r_max, n_slices))
    R = n_slices * r_max

    def normal(shape, std):
        return (torch.randn(shape, generator=g) * std).to(BF16)
    mag = torch.rand((T, O), generator=g) * 1.5 + 0.5
    sign = torch.randint(0, 2, (T, O), generator=g).float() * 2 - 1
    return dict(x=normal((T, K), 1.0), A=normal((N_ADAPTERS, R, K), K ** -0.5),
                B=normal((N_ADAPTERS, O, r_max), 0.02 * r_max ** -0.5),
                out=(mag * sign).to(BF16),
                scale=torch.tensor(SCALES, dtype=torch.float32),
                slices=SLICES[(O, n_slices)], idx=adapter_idx_of(T))


def ref_out(case):
    """The reference result of shrink + expand on a case (CPU)."""
    out = case["out"].clone()
    y = ref.lora_shrink(case["x"], case["A"], case["idx"])
    ref.lora_expand_add_(out, y, case["B"], case["scale"], case["slices"],
                         case["idx"])
    return y, out


def shuffled_ref_out(case, seed=0):
    """The same reference evaluated in another summation order: K and the
    rank axis of every slice permuted (the math is unchanged)."""
    g = torch.Generator().manual_seed(seed)
    K = case["x"].shape[1]
    r_max = case["B"].shape[2]
    n_slices = len(case["slices"])
    pk = torch.randperm(K, generator=g)
    pr = torch.randperm(r_max, generator=g)
    pR = torch.cat([s * r_max + pr for s in range(n_slices)])
    shuffled = dict(case, x=case["x"][:, pk].contiguous(),
                    A=case["A"][:, pR][:, :, pk].contiguous(),
                    B=case["B"][:, :, pr].contiguous())
    return ref_out(shuffled)[1]


def bf16_ulp_distance(a, b):
    """Element-wise distance in bf16 steps (0 = same bits, 1 = adjacent
    values; +0 and -0 coincide)."""
    def ordered(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7fff), bits)
    return (ordered(a) - ordered(b)).abs()


# ------------------------------------------------------------ adapters
MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
           "down_proj")


def random_adapter(model, r, targets=MODULES, seed=0, std=0.05, zero_b=False):
    """PEFT-named LoRA tensors for ``model`` -> (r, lora_alpha, targets,
    weights) as ``model.add_adapter`` takes them."""
    g = torch.Generator().manual_seed(seed)
    geo = model._lora_geometry()
    weights = {}
    for i in range(model.config.n_layers):
        for m in targets:
            proj, s = model._LORA_MODULES[m]
            K, widths = geo[proj]
            a = torch.randn((r, K), generator=g) * std
            b = torch.randn((widths[s], r), generator=g) * std
            if zero_b:
                b.zero_()
            weights[model._peft_key(i, m, "A")] = a.to(model.dtype)
            weights[model._peft_key(i, m, "B")] = b.to(model.dtype)
    return r, 2.0 * r, list(targets), weights


def merged_model(model, name, make_model):
    """A copy of ``model`` (built by ``make_model()``) whose weights are
    W + scale * B @ A for adapter ``name``."""
    merged = make_model()
    src = model._adapter_src[name]
    scale = src["lora_alpha"] / src["r"]
    geo = model._lora_geometry()
    for i in range(model.config.n_layers):
        for m in src["target_modules"]:
            proj, s = model._LORA_MODULES[m]
            _, widths = geo[proj]
            lo = sum(widths[:s])
            a = src["tensors"][model._peft_key(i, m, "A")].float()
            b = src["tensors"][model._peft_key(i, m, "B")].float()
            w = merged.params[f"l{i}.{proj}"]
            w[lo:lo + widths[s]] += (scale * (b @ a)).to(w.dtype)
    return merged
