"""CPU: the gradient acceptance rule of tests/_zoo.py (check_gradients), the correctness bar of a
whole model, on hand-made gradients whose errors are exact by construction.

Every tensor has two elements: the float64 gradient is [n64, 0], the float32 CPU run [n64, ec] and
the device's [n64, eh], so the three norms the rule reads are n64, ec and eh to the bit.

The rule's two parts cannot both sit at their edge: were EVERY tensor at 4 * ec + 1e-3 * n64, the
global error would be at least sqrt(16 a^2 + 1e-6) for a = the CPU-fp32 global error, which is above
3 a + 1e-4 for every a.  So the per-tensor edge is tested on nine light tensors next to one heavy,
exact tensor that carries the global norm, and the global edge with tensors that are all inside
their own bounds."""
import pytest
import torch

from _zoo import check_gradients

HEAVY = (2.0 ** 20, 1.0, 0.0)   # n64, ec, eh: carries the global norm, no device error
N, EC = 1.0, 2.0 ** -10         # the light tensors
BOUND = 4 * EC + 1e-3 * N


def _case(rows):
    params, g64, g32 = {}, {}, {}
    for i, (n64, ec, eh) in enumerate(rows):
        k = "t%d" % i
        g64[k] = torch.tensor([n64, 0.0], dtype=torch.float64)
        g32[k] = torch.tensor([n64, ec], dtype=torch.float32)
        params[k] = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))
        params[k].grad = torch.tensor([n64, eh], dtype=torch.float64)
    return params, g64, g32


def _light(*eh):
    return [HEAVY] + [(N, EC, e) for e in eh]


def test_every_light_tensor_exactly_at_the_bound_passes():
    table = check_gradients(*_case(_light(*[BOUND] * 9)))
    assert [w[0] for w in table] == [1.0] * 9 + [0.0]  # at the bound is not beyond it


def test_one_of_ten_beyond_the_bound_but_under_the_cap_passes():
    table = check_gradients(*_case(_light(4 * EC + 2.9e-2 * N, *[0.5 * BOUND] * 8)))
    assert table[0][0] > 1.0 >= table[1][0]


def test_two_of_ten_beyond_the_bound_fail():
    with pytest.raises(AssertionError):
        check_gradients(*_case(_light(*[1.01 * BOUND] * 2, *[0.5 * BOUND] * 7)))


def test_one_tensor_beyond_the_cap_fails():
    with pytest.raises(AssertionError):
        check_gradients(*_case(_light(4 * EC + 3.1e-2 * N, *[0.5 * BOUND] * 8)))


@pytest.mark.parametrize("factor,passes", [(1 - 1e-6, True), (1 + 1e-6, False)])
def test_global_error_just_beyond_three_times_cpu_plus_1e_4_fails(factor, passes):
    """Ten tensors of equal relative error r and an exact CPU run (nc = 0): the global error is r,
    every tensor is far inside its own bound (r / 1e-3), and the edge is r = 1e-4."""
    rows = [(n64, 0.0, 1e-4 * factor * n64) for n64 in (1.0, 2.0, 4.0, 8.0, 16.0) * 2]
    if passes:
        assert max(w[0] for w in check_gradients(*_case(rows))) < 0.11
    else:
        with pytest.raises(AssertionError):
            check_gradients(*_case(rows))


def test_a_used_parameter_without_a_gradient_fails():
    params, g64, g32 = _case(_light(*[0.5 * BOUND] * 9))
    params["t3"].grad = None
    with pytest.raises(AssertionError):
        check_gradients(params, g64, g32)
    params, g64, g32 = _case(_light(*[0.5 * BOUND] * 9))
    params["extra"] = torch.nn.Parameter(torch.zeros(2))  # one the oracle has no gradient for
    with pytest.raises(AssertionError):
        check_gradients(params, g64, g32)


def test_an_unused_parameter_must_have_no_gradient():
    params, g64, g32 = _case(_light(*[0.5 * BOUND] * 9))
    params["dead.weight"] = torch.nn.Parameter(torch.zeros(2))
    unused = lambda k: k.startswith("dead.")  # noqa: E731
    check_gradients(params, g64, g32, unused)
    params["dead.weight"].grad = torch.zeros(2)  # a zero gradient is a gradient
    with pytest.raises(AssertionError):
        check_gradients(params, g64, g32, unused)
