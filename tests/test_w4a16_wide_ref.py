"""The wide int4 ops on CPU tensors are the reference ops, and the routing
table names only shapes the wide kernel takes, in rows it takes."""

import pytest
import torch

from resilient_llm_amd import ops
from resilient_llm_amd.models import LlamaForCausalLM, get_config

import awq_cases
import w4a16_cases


@pytest.mark.parametrize("shape", [(129, 128, 256), (512, 256, 128)])
def test_wide_ops_on_cpu_equal_the_oracle(shape):
    case = w4a16_cases.exact_case(*shape)
    out = torch.empty_like(case.expected)
    assert ops.w4a16_wide_linear(case.x, case.packed, case.s, out=out) is out
    assert torch.equal(out, case.expected)
    zp = awq_cases.exact_case(*shape)
    assert torch.equal(ops.w4a16_zp_wide_linear(zp.x, zp.packed, zp.meta),
                       zp.expected)


def test_routing_table_shape():
    table = LlamaForCausalLM._W4_WIDE_ROWS_BY_SHAPE
    for (N, K), (first, last) in table.items():
        assert N % 128 == 0 and K % 128 == 0
        assert 64 < first <= last <= 512
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device="cpu", dtype=torch.float32, seed=1)
    assert not set(model._w4_shapes().values()) & set(table)
