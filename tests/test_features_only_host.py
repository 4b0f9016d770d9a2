"""CPU (-m "not gpu"): a feature layer WITHOUT alignment - ``pp.PreprocessingANN(None, feature_layer)`` /
``pp.AlignFeatureLayer(n, None, None, features)`` (CVF_PP_FEATURES, csrc/k1_features.hip).  Host side only: construction, the
tables the kernels read, the torch twin of the export against ``oracle.pp.features_of`` in fp64, and the C-ABI surface."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.synth import make_molecule_traj
from tests.test_host_logic import built_lib, header_functions  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]
# 70 atoms, a list that reads atoms 0, 64 and 69 (the first atom, the first past a 64-atom frame, the last)
WIDE70 = [("position", (69, 0, 64)), ("bond", (0, 69)), ("angle", (64, 0, 33)), ("dihedral", (0, 64, 69, 12)), ("bond", (64, 65))]

TABLES = ("rec", "rec_slot", "slot_atom", "atom_slot", "mrec", "slot_row")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def plain(n_atoms, feats, angle_value=False):
    from colvarsfinder import pp
    return pp.AlignFeatureLayer(n_atoms, None, None, feats, angle_value)


def test_both_constructors_build_the_layer():
    from colvarsfinder import pp
    atoms = types.SimpleNamespace(ix=np.arange(100, 110))
    feats = [pp.Feature("p", "position", 100 + np.array([0, 2, 3, 5])), pp.Feature("b", "bond", [100, 101]),
             pp.Feature("a", "angle", [101, 102, 103]), pp.Feature("d", "dihedral", [104, 105, 106, 107])]
    fl = pp.FeatureLayer(feats, atoms, use_angle_value=False)
    a = pp.PreprocessingANN(None, fl)
    b = plain(10, [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("angle", (1, 2, 3)), ("dihedral", (4, 5, 6, 7))])
    assert isinstance(a, pp.AlignFeatureLayer) and not a.aligned and not b.aligned
    assert a.d_r == b.d_r == fl.output_dimension() == 12 + 1 + 1 + 2
    assert a.features == b.features and a.n_atoms == b.n_atoms == 10
    for t in TABLES:
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    assert a.align_idx.numel() == 0 and a.ref_c.numel() == 0 and a.align_w is None
    assert a.derivative_table_limits() is None


@pytest.mark.parametrize("n_atoms,feats", [(10, MIXED), (70, WIDE70)])
@pytest.mark.parametrize("angle_value", [False, True])
def test_tables_are_those_of_the_aligned_constructor(n_atoms, feats, angle_value):
    from colvarsfinder import pp
    _, _, ref = make_molecule_traj(n_atoms, 2, seed=1)
    free = plain(n_atoms, feats, angle_value)
    aligned = pp.AlignFeatureLayer(n_atoms, [0, 1, 2, 4], ref[[0, 1, 2, 4]], feats, angle_value)
    assert aligned.aligned and not free.aligned
    assert free.d_r == aligned.d_r and free.features == aligned.features and free.use_angle_value == aligned.use_angle_value
    for t in TABLES:
        assert torch.equal(getattr(free, t), getattr(aligned, t)), t
    assert (free._n_slot, free._n_rec_slot, free._n_ref) == (aligned._n_slot, aligned._n_rec_slot, aligned._n_ref)
    assert free._flags == 0   # the structure hints describe alignment layouts


def test_alignment_arguments_without_alignment_assert():
    from colvarsfinder import pp
    with pytest.raises(AssertionError, match="align_weights"):
        pp.AlignFeatureLayer(10, None, None, MIXED, False, align_weights=np.ones(3))
    with pytest.raises(AssertionError, match="ref_pos"):
        pp.AlignFeatureLayer(10, None, np.zeros((3, 3)), MIXED)
    with pytest.raises(AssertionError, match="out of range"):
        plain(5, [("bond", (0, 5))])
    # the aligned form keeps its own assertions, word for word
    with pytest.raises(AssertionError, match="at least 3 atoms are needed for the alignment"):
        pp.AlignFeatureLayer(10, [0, 1], np.zeros((2, 3)), MIXED)


def test_limits_of_the_new_kernels_are_reported():
    from colvarsfinder import _hip
    n = _hip.FEATURES_MAX_SLOT + 2
    assert plain(n, [("position", tuple(range(n - 2)))]).derivative_table_limits() is None
    why = plain(n, [("position", tuple(range(n - 1)))]).derivative_table_limits()
    assert why is not None and "n_slot" in why and str(_hip.FEATURES_MAX_SLOT) in why
    bonds = [("bond", (i, i + 1)) for i in range(_hip.FEATURES_MAX_REF // 2 + 1)]
    why = plain(len(bonds) + 1, bonds).derivative_table_limits()
    assert why is not None and "n_ref" in why and str(_hip.FEATURES_MAX_REF) in why
    # the lists the kernels must take: config 5's (128 dihedrals + 128 bonds over 5000 atoms) and 64 positions
    rs = np.random.RandomState(5)
    c5 = [("dihedral", tuple(int(i) for i in rs.choice(5000, 4, replace=False))) for _ in range(128)] + \
         [("bond", tuple(int(i) for i in rs.choice(5000, 2, replace=False))) for _ in range(128)]
    layer = plain(5000, c5)
    assert layer.d_r == 384 and layer._n_ref == 768 and layer.derivative_table_limits() is None
    assert plain(64, [("position", tuple(range(64)))]).derivative_table_limits() is None


def reference(x64, feats, angle_value):
    from oracle.pp import features_of
    return features_of(x64, feats, angle_value)


@pytest.mark.parametrize("n_atoms,feats", [(10, MIXED), (70, WIDE70)])
@pytest.mark.parametrize("angle_value", [False, True])
def test_torch_twin_reproduces_features_of(n_atoms, feats, angle_value):
    from colvarsfinder.export import ScriptableAlignFeature
    traj, _, _ = make_molecule_traj(n_atoms, 33, seed=40 + n_atoms)
    x = torch.tensor(traj, dtype=torch.float64)
    twin = ScriptableAlignFeature(plain(n_atoms, feats, angle_value))
    got, want = twin(x), reference(x, feats, angle_value)
    assert got.dtype == torch.float64 and got.shape == want.shape
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    # position outputs are the coordinates themselves
    t, atoms = feats[0]
    assert t == "position" and torch.equal(got[:, :3 * len(atoms)], x[:, list(atoms)].reshape(len(x), -1))


@pytest.mark.parametrize("angle_value", [False, True])
def test_scripted_twin_and_its_double_backward(angle_value, tmp_path):
    from colvarsfinder.export import ScriptableAlignFeature
    traj, _, _ = make_molecule_traj(10, 9, seed=77)
    twin = torch.jit.script(ScriptableAlignFeature(plain(10, MIXED, angle_value)))
    path = str(tmp_path / "twin.pt")
    twin.save(path)
    twin = torch.jit.load(path)
    c = torch.randn(20, generator=torch.Generator().manual_seed(1), dtype=torch.float64)   # (d_r is 20 or 18)

    def second(f):
        x = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        y = f(x)
        (g,) = torch.autograd.grad((y * c[:y.shape[1]]).sum(), x, create_graph=True)
        (h,) = torch.autograd.grad((g * g).sum(), x)
        return y.detach(), g.detach(), h

    got, want = second(twin), second(lambda x: reference(x, MIXED, angle_value))
    for a, b, what in zip(got, want, ("value", "gradient", "second derivative")):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-10 * float(b.abs().max()), err_msg=what)


def test_c_abi_surface(built_lib):  # noqa: F811
    from colvarsfinder import _hip
    header = open(os.path.join(ROOT, "include", "cvf.h")).read()
    modes = dict(re.findall(r"(CVF_PP_(?:IDENTITY|ALIGN|FACTORED|FEATURES)) = (\d+)", header))
    assert int(modes["CVF_PP_FEATURES"]) == _hip.PP_FEATURES == 3
    assert (int(modes["CVF_PP_IDENTITY"]), int(modes["CVF_PP_ALIGN"]), int(modes["CVF_PP_FACTORED"])) == \
        (_hip.PP_IDENTITY, _hip.PP_ALIGN, _hip.PP_FACTORED)
    limits = {k: int(v) for k, v in re.findall(r"#define (CVF_FEATURES_MAX_(?:SLOT|REF)) (\d+)", header)}
    assert limits == {"CVF_FEATURES_MAX_SLOT": _hip.FEATURES_MAX_SLOT, "CVF_FEATURES_MAX_REF": _hip.FEATURES_MAX_REF}
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    for name in header_functions():
        assert hasattr(handle, name), f"{name} declared in include/cvf.h but not exported"
    assert sorted(_hip.EXPORTED_SYMBOLS) == header_functions()
