"""CPU (-m "not gpu"): the oracle is pinned to the reference's fixtures with decoder and regulariser nets of different depths
(tests/golden/train_regae_depth_*, written by tools/gen_golden.py --regae-depth-only) - tests/test_oracle_golden.py's
test_regae_train_trace itself on the new names: known answers and gradients at the initial weights and the training trace, 1e-9 in
fp64."""
import pytest
import torch

from tests import goldens
from tests import test_oracle_golden as O

FIXTURES = ("train_regae_depth_id2_k2", "train_regae_depth_mol10_k2", "train_regae_depth_id2_k1_gen")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_is_pinned_to_the_depth_fixtures(name, tag):
    g = goldens.load(name, tag)
    e, d, r = ([int(v) for v in g[k]] for k in ("e_dims", "d_dims", "r_dims"))
    assert len(d) != len(r) and e[-1] == d[0] == r[0] and e[0] == d[-1] and r[-1] == 1
    assert (int(g["lag_reg"]) == 0) == name.endswith("_gen") and 200 <= g["traj"].shape[0] <= 600
    assert O.TOL["f64"] == dict(rtol=1e-9, atol=1e-11)
    O.test_regae_train_trace(name, tag)


def test_fixture_shapes_are_the_ones_asked_for():
    dims = {n: tuple([int(v) for v in goldens.load(n, "f64")[k]] for k in ("e_dims", "d_dims", "r_dims")) + (int(goldens.load(n, "f64")["K"]),)
            for n in FIXTURES}
    assert dims["train_regae_depth_id2_k2"] == ([2, 12, 12, 2], [2, 12, 12, 2], [2, 12, 1], 2)                 # the decoder is deeper
    assert dims["train_regae_depth_mol10_k2"] == ([30, 20, 20, 20, 2], [2, 10, 30], [2, 10, 10, 1], 2)         # the regularisers are deeper
    old = goldens.load("train_regae_id2_k1_gen", "f64")
    assert dims["train_regae_depth_id2_k1_gen"] == ([int(v) for v in old["e_dims"]], [1, 20, 2], [int(v) for v in old["r_dims"]], 1)
