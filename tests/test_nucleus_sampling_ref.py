"""ref.sample_nucleus (what ops.sample_nucleus runs on CPU tensors) against
the float64 definition the GPU test uses."""

import pytest

from resilient_llm_amd.ops import ref
from tests.test_nucleus_sampling_gpu import _case, _oracle, _run


@pytest.mark.parametrize("kind", ["p0.5", "both", "all", "hist300", "tie"])
def test_greedy_is_exact_and_draws_stay_in_the_kept_set(kind):
    for combo in range(3):
        c = _case(1003, kind, combo)
        z, keep = _oracle(c)
        drawn = [set() for _ in c["rows"]]
        for c["step"] in range(12):
            _, got = _run(c, dev="cpu")
            for r, t in enumerate(got.tolist()):
                assert keep[r, t]
                drawn[r].add(t)
        for r, row in enumerate(c["rows"]):
            T = c["temps"][row]
            if T <= 0:        # float64 arg-max of the penalised z, lowest index
                assert drawn[r] == {int((z[r] == z[r].max()).nonzero()[0])}
            elif kind == "tie" and T <= 1:     # every tied token is drawable
                assert drawn[r] == {1, 3, 5}


def test_top_p_one_without_penalties_is_sample_constrained():
    for combo in range(3):
        args, got = _run(_case(1003, "off", combo), dev="cpu")
        want = ref.sample_constrained(*args[:7], *args[10:13])
        assert got.tolist() == want.tolist()

