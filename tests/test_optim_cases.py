"""CPU (-m "not gpu"): the tables of the optimiser tests stay tied to what they were derived from - the bars of the full-pack
forward cases to the fp32 CPU evaluation (tests/optim_inputs.py), the learning rates of the SGD traces (tests/optim_tasks.py)
to the distance the fp64 oracle's parameters travel."""
import pytest

from tests import optim_cases as OC
from tests import optim_tasks as O


def test_forward_bars_are_tied_to_the_fp32_evaluation():
    """optim_cases.FWD_BARS (tests/test_optimizer_gpu.py::test_full_pack_forward_vs_fp64): 8 x the worst distance of the pinned
    fp32 evaluation from the fp64 nets over FWD_CASES, as recomputed here: between 4 x and 16 x."""
    from tests import optim_inputs as I
    assert len(OC.FWD_CASES) == 80 and {nh for _, nh in OC.FWD_SHAPES} == {1, 2, 3, 4, 5} and set(OC.FWD_SHAPES) <= set(OC.EF_SHAPES)
    for what, bar, e in zip(("y", "g"), OC.FWD_BARS, I.fwd_worst_e32()):
        assert 4 * e <= bar <= 16 * e, f"{what}: bar {bar:.2e}, worst e32 {e:.2e}"


@pytest.mark.parametrize("case", O.CASES, ids=[c.id for c in O.CASES])
def test_sgd_cases_move_the_oracle(case):
    """Every trainable tensor of the fp64 oracle ends at least 100 x the parameter bar from where it started (and the run stays
    finite), so that a step that updates nothing, or not every tensor, fails tests/test_optimizer_tasks_gpu.py."""
    import numpy as np
    trace = O.oracle_trace(case)
    assert np.isfinite(trace["train"]).all() and np.isfinite(trace["test"]).all()
    assert trace["train"].shape[:2] == (O.EPOCHS, 3) and trace["test"].shape[:2] == (O.EPOCHS, 1)
    assert O.BARS[case.id][1] <= O.CEILING and O.BARS[case.id][0] <= O.CEILING
    assert O.movement(case, trace) >= O.MOVE_FACTOR * O.BARS[case.id][1], O.movement(case, trace)
    for n in trace["final"]:
        if O.unmoved(case, n) and case.kind == "regae" and n.startswith("encoder."):
            assert (trace["final"][n] == trace["initial"][n]).all()
