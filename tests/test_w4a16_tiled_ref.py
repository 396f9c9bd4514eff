"""The tiled int4 ops on CPU tensors are the reference ops, which take any
M: equal to the float64 oracle rounded once to bf16 on exact-integer
cases past 64 rows."""

import pytest
import torch

from resilient_llm_amd import ops

import awq_cases
import w4a16_cases


@pytest.mark.parametrize("shape", [(65, 64, 128), (256, 128, 512)])
def test_tiled_ops_on_cpu_equal_the_oracle(shape):
    case = w4a16_cases.exact_case(*shape)
    want = w4a16_cases.oracle64(case.x, case.q, case.s).float().to(
        torch.bfloat16)
    assert torch.equal(ops.w4a16_tiled_linear(case.x, case.packed, case.s),
                       want)
    out = torch.empty_like(want)
    assert ops.w4a16_tiled_linear(case.x, case.packed, case.s, out=out) is out
    assert torch.equal(out, want)
    zp = awq_cases.exact_case(*shape)
    want = awq_cases.oracle64(zp.x, zp.u, zp.z, zp.s).float().to(
        torch.bfloat16)
    assert torch.equal(ops.w4a16_zp_tiled_linear(zp.x, zp.packed, zp.meta),
                       want)
