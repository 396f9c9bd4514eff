"""ref.sample_constrained (the CPU path of ops.sample_constrained)
against the float64 definition: z = logit + bias, kept = {z >= k-th
largest z} & {z >= z_max + T*ln(min_p)}, greedy = arg-max z (lowest
index).  Stochastic rows are checked for kept-set membership over many
seeds and for determinism in (seeds, step), not for a stream."""

import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref

V = 96


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _logits(B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 33, (B, V), generator=g) * 0.25).to(
        torch.bfloat16)


def _call(lg, rows, temps, seeds, step, ks, ms, biases):
    offs, ids, vals = [0], [], []
    for b in biases:
        ids += [i for i, _ in b]
        vals += [v for _, v in b]
        offs.append(len(ids))
    return ops.sample_constrained(
        lg, _i32(rows), torch.tensor(temps, dtype=torch.float32),
        torch.tensor(seeds, dtype=torch.int64), step, _i32(ks),
        torch.tensor(ms, dtype=torch.float32), _i32(offs), _i32(ids),
        torch.tensor(vals, dtype=torch.float32)).tolist()


def _kept(lg_row, T, k, m, bias):
    z = lg_row.double().clone()
    for i, v in bias:
        z[i] += v
    keep = torch.ones(V, dtype=torch.bool)
    if 1 <= k < V:
        keep &= z >= z.sort(descending=True).values[k - 1]
    if m > 0:
        cut = z.max() + T * math.log(m)
        assert (z - cut).abs().min() > 0.12
        keep &= z >= cut
    return z, keep


def test_dispatches_to_ref_on_cpu():
    assert ops.sample_constrained.__module__ == "resilient_llm_amd.ops"
    assert callable(ref.sample_constrained)


def test_greedy_exact_with_bias():
    lg = _logits()
    bias = [[0, 8.0], [17, -8.0], [V - 1, 8.0]]
    got = _call(lg, [0, 1, 2, 3], [0.0] * 4, [1, 2, 3, 4], 0,
                [1, 5, 0, V + 3], [0.0, 0.5, 0.0, 0.9],
                [bias, [], bias, []])
    for r in range(4):
        z, _ = _kept(lg[r], 0.0, 0, 0.0, bias if r % 2 == 0 else [])
        assert got[r] == int((z == z.max()).nonzero()[0])


@pytest.mark.parametrize("k,n,bias", [
    (1, None, []), (5, None, []), (0, 3, []), (7, 5, [[2, 4.0], [50, -8.0]]),
    (V - 1, None, []),
])
def test_kept_set_membership_over_seeds(k, n, bias):
    lg = _logits()
    T = 0.5
    m = math.exp(-(n + 0.5) * 0.25 / T) if n is not None else 0.0
    z, keep = _kept(lg[1], T, k, m, bias)
    seen = set()
    for seed in range(60):
        tok = _call(lg, [1], [1.0, T, 1.0, 1.0], [0, seed, 0, 0], seed % 3,
                    [k], [m], [bias])[0]
        assert keep[tok], (tok, k, m)
        seen.add(tok)
    if keep.sum() > 1 and k != 1:
        assert len(seen) > 1                 # it does sample


def test_off_values_equal_plain_distribution_support():
    lg = _logits()
    # k == 0, k == V, k > V and m == 0 all keep everything: same draw as
    # the unconstrained reference sampler with the same generator seed
    temps, seeds = [0.7] * 4, [5, 6, 7, 8]
    plain = ref.sample(lg, torch.tensor(temps), torch.tensor(seeds), 2).tolist()
    for k in (0, V, V + 9):
        got = _call(lg, [0, 1, 2, 3], temps, seeds, 2, [k] * 4, [0.0] * 4,
                    [[]] * 4)
        assert got == plain


def test_boundary_ties_all_stay():
    lg = _logits().clone()
    lg[0, [4, 40, 80]] = 9.0                 # three-way tie at the top
    seen = {_call(lg, [0], [1.0] * 4, [s, 0, 0, 0], 0, [2], [0.0], [[]])[0]
            for s in range(80)}
    assert seen == {4, 40, 80}


def test_deterministic_in_seed_and_step():
    lg = _logits()
    args = ([2, 0, 2], [1.0] * 4, [11, 12, 13, 14])
    a = _call(lg, *args, 4, [10] * 3, [0.0] * 3, [[]] * 3)
    b = _call(lg, *args, 4, [10] * 3, [0.0] * 3, [[]] * 3)
    assert a == b and a[0] == a[2]           # a repeated row repeats
    draws = {tuple(_call(lg, *args, s, [10] * 3, [0.0] * 3, [[]] * 3))
             for s in range(12)}
    assert len(draws) > 1                    # the step enters the stream
    # seeds + GOLDEN*step is the contract: (seed, step) == (seed', 0)
    C = 0x9e3779b97f4a7c15
    shifted = [((s + C * 4 + 2 ** 63) % 2 ** 64) - 2 ** 63
               for s in (11, 12, 13, 14)]
    assert _call(lg, [2, 0, 2], [1.0] * 4, shifted, 0, [10] * 3, [0.0] * 3,
                 [[]] * 3) == a


def test_empty_selection_and_mismatches():
    lg = _logits()
    out = ops.sample_constrained(
        lg, _i32([]), torch.ones(4), torch.zeros(4, dtype=torch.int64), 0,
        _i32([]), torch.zeros(0), _i32([0]), _i32([]), torch.zeros(0))
    assert out.shape == (0,) and out.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.sample_constrained(
            lg, _i32([0]), torch.ones(4), torch.zeros(4, dtype=torch.int64),
            0, _i32([0, 0]), torch.zeros(1), _i32([0, 0]), _i32([]),
            torch.zeros(0))
    with pytest.raises(ValueError):
        ops.sample_constrained(
            lg, _i32([0]), torch.ones(4), torch.zeros(4, dtype=torch.int64),
            0, _i32([0]), torch.zeros(1), _i32([0, 1]), _i32([3]),
            torch.zeros(0))
