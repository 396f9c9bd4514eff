"""The SwiGLU-fused int4 ops on CPU tensors: the composition of the
existing reference functions, and the argument checks of the device ops."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.ops import ref

import awq_cases
import w4a16_cases
from w4a16_cases import BF16


def forms(N, K):
    """(fused op, plain reference, packed, s or meta) of both forms."""
    sym = w4a16_cases.random_case(1, N, K)
    zp = awq_cases.random_case(1, N, K)
    return [(ops.w4a16_silu_linear, ref.w4a16_linear, sym.packed, sym.s),
            (ops.w4a16_zp_silu_linear, ref.w4a16_zp_linear, zp.packed,
             zp.meta)]


def test_cpu_ops_are_the_composed_references():
    gu = (4 * torch.randn(3, 512, generator=torch.Generator().manual_seed(1))
          ).to(BF16)
    for fused, plain, packed, sm in forms(64, 256):
        want = plain(ref.silu_mul(gu), packed, sm)
        assert torch.equal(fused(gu, packed, sm), want)
        out = torch.empty_like(want)
        assert fused(gu, packed, sm, out=out) is out
        assert torch.equal(out, want)


# (M, gu width, dtype, ws elements) against K = 256, splitk = 2
@pytest.mark.parametrize("M,width,dtype,n_ws", [
    (3, 511, BF16, None), (3, 768, BF16, None), (0, 512, BF16, None),
    (65, 512, BF16, None), (3, 512, torch.float32, None), (3, 512, BF16, 8)])
def test_argument_checks_on_cpu(M, width, dtype, n_ws):
    for fused, _, packed, sm in forms(64, 256):
        ws = None if n_ws is None else torch.empty(n_ws)
        with pytest.raises(ValueError):
            fused(torch.zeros(M, width, dtype=dtype), packed, sm, 2, ws=ws)
        # the same call with a valid gu and a slab that is large enough
        fused(torch.zeros(3, 512, dtype=BF16), packed, sm, 2,
              ws=torch.empty(2 * 3 * 64))
