"""ref.token_logprobs (the CPU path of ops.token_logprobs) against an
independent float64 computation."""

import math

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref


def _float64(logits, rows, tokens, k):
    """Per-row python/float64 reference: value descending, index
    ascending on ties."""
    chosen, top_v, top_i = [], [], []
    for r, t in zip(rows, tokens):
        x = logits[r].double()
        lse = torch.logsumexp(x, 0)
        lp = (x - lse).tolist()
        order = sorted(range(len(lp)), key=lambda j: (-lp[j], j))[:k]
        chosen.append(lp[t])
        top_v.append([lp[j] for j in order])
        top_i.append(order)
    return chosen, top_v, top_i


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,k", [
    ([0, 1, 2, 3], 5),
    ([2], 20),                # subset
    ([3, 0, 3, 1], 3),        # out of order, with repeats
    ([1, 2], 0),              # k = 0
])
def test_matches_float64(dtype, rows, k):
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(4, 257, generator=g) * 4).to(dtype)
    tokens = [(7 * i + 3) % 257 for i in range(len(rows))]
    c, v, i = ops.token_logprobs(
        logits, torch.tensor(rows, dtype=torch.int32),
        torch.tensor(tokens, dtype=torch.int32), k)
    assert c.shape == (len(rows),) and c.dtype == torch.float32
    assert v.shape == (len(rows), k) and v.dtype == torch.float32
    assert i.shape == (len(rows), k) and i.dtype == torch.int32
    wc, wv, wi = _float64(logits, rows, tokens, k)
    assert i.tolist() == wi
    assert torch.allclose(c.double(), torch.tensor(wc, dtype=torch.float64),
                          atol=1e-5, rtol=0)
    if k:
        assert torch.allclose(v.double(),
                              torch.tensor(wv, dtype=torch.float64),
                              atol=1e-5, rtol=0)


def test_all_equal_row_tie_order():
    V, k = 300, 20
    logits = torch.full((2, V), 1.5, dtype=torch.bfloat16)
    c, v, i = ref.token_logprobs(logits, torch.tensor([1], dtype=torch.int32),
                                 torch.tensor([17], dtype=torch.int32), k)
    assert i[0].tolist() == list(range(k))
    assert torch.allclose(v[0], torch.full((k,), -math.log(V)), atol=1e-6)
    assert abs(c[0].item() + math.log(V)) < 1e-6


def test_rejects_bad_k_and_lengths():
    logits = torch.zeros(2, 8)
    r = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ref.token_logprobs(logits, r, r, 21)
    with pytest.raises(ValueError):
        ref.token_logprobs(logits, r, r, 9)        # k > V
    with pytest.raises(ValueError):
        ref.token_logprobs(logits, r, torch.zeros(2, dtype=torch.int32), 1)
