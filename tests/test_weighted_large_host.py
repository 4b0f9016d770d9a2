"""CPU: the opt-in ``weights_any_size=True`` of the preprocessing layer (per-atom alignment weights on frames of more than 64
atoms) - descriptor tables and flags, the unchanged default, the molann-style constructors, and the torch twin against the oracle."""
import numpy as np
import pytest
import torch

from tests.synth import make_molecule_traj
from tests.weighted_large_cases import NOT_IGNORED, frames, oracle_features, position_columns, weights_for

MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]


@pytest.mark.parametrize("n_atoms,contig", [(80, True), (80, False), (256, True), (256, False)])
def test_weighted_layer_of_any_size_tables_and_flags(n_atoms, contig):
    from colvarsfinder import _hip, pp
    _, _, ref = frames(n_atoms, 2, seed=n_atoms)
    align = list(range(n_atoms)) if contig else sorted(np.random.RandomState(3).choice(n_atoms, n_atoms // 2, replace=False).tolist())
    w = weights_for(n_atoms, len(align))
    feats = [("position", tuple(range(n_atoms)))] if contig else MIXED
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, align_weights=w, weights_any_size=True)
    # the flags describe the tables, not the weights; PURE_POSITION is meaningless on the streaming path
    assert layer._flags == (_hip.PP_ALIGN_CONTIG if contig else 0) | _hip.PP_SLOT_BATCHED
    aw = layer.align_w.double().numpy()
    assert aw.shape == (len(align),) and aw.dtype == np.float64
    np.testing.assert_allclose(aw.mean(), 1.0, rtol=1e-6)
    np.testing.assert_allclose(aw, w * len(w) / w.sum(), rtol=1e-6)
    # ref_c = w_hat (ref - weighted centroid): sums to zero, and divides back to the centred reference
    rc = layer.ref_c.double().numpy()
    assert np.abs(rc.sum(0)).max() <= 1e-5 * np.abs(rc).sum(0).max()
    what = w * len(w) / w.sum()
    want = what[:, None] * (ref[align] - (what[:, None] * ref[align]).mean(0, keepdims=True))
    np.testing.assert_allclose(rc, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    assert layer.n_atoms == n_atoms and layer.align_idx.tolist() == align and layer.rec_slot.shape[0] % 64 == 0
    assert layer._n_rec_slot == layer.rec_slot.shape[0] and layer._n_slot == layer.slot_atom.numel()
    assert layer.derivative_table_limits() is None


def test_option_changes_nothing_on_small_frames_and_default_still_refuses():
    from colvarsfinder import pp
    _, _, ref = make_molecule_traj(80, 4, seed=3)
    w = weights_for(10, 6)
    a = pp.AlignFeatureLayer(10, [0, 1, 2, 4, 5, 8], ref[[0, 1, 2, 4, 5, 8]], MIXED, align_weights=w)
    b = pp.AlignFeatureLayer(10, [0, 1, 2, 4, 5, 8], ref[[0, 1, 2, 4, 5, 8]], MIXED, align_weights=w, weights_any_size=True)
    assert a._flags == b._flags == 0
    for name in ("align_w", "ref_c", "rec", "rec_slot", "mrec", "slot_row"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    with pytest.raises(AssertionError, match="at most 64 atoms"):
        pp.AlignFeatureLayer(80, list(range(80)), ref, [("position", tuple(range(80)))], False, align_weights=np.ones(80))
    with pytest.raises(AssertionError, match="at most 64 atoms"):
        pp.AlignFeatureLayer(80, list(range(80)), ref, [("position", tuple(range(80)))], False, align_weights=np.ones(80),
                             weights_any_size=False)
    # an unweighted layer is not touched by the option
    u = pp.AlignFeatureLayer(80, list(range(80)), ref, [("position", tuple(range(80)))], weights_any_size=True)
    v = pp.AlignFeatureLayer(80, list(range(80)), ref, [("position", tuple(range(80)))])
    assert u._flags == v._flags and u.align_w is None and torch.equal(u.ref_c, v.ref_c)


def test_alignment_layer_and_preprocessing_ann_forward_the_option():
    from colvarsfinder import pp

    class Group:
        def __init__(self, ix, positions):
            self.ix, self.positions = np.asarray(ix), np.asarray(positions)

    n = 90
    _, _, ref = frames(n, 2, seed=9)
    ix = np.arange(100, 100 + n)
    align_ix = ix[5:75]
    w = weights_for(n, len(align_ix))
    feats = [pp.Feature("p", "position", ix[[3, 40, 80]]), pp.Feature("b", "bond", ix[[1, 2]])]
    fl = pp.FeatureLayer(feats, Group(ix, ref))
    with pytest.raises(AssertionError, match="at most 64 atoms"):
        pp.PreprocessingANN(pp.AlignmentLayer(Group(align_ix, ref[5:75]), Group(ix, ref), weights=w), fl)
    al = pp.AlignmentLayer(Group(align_ix, ref[5:75]), Group(ix, ref), weights=w, weights_any_size=True)
    assert al.weights_any_size is True
    layer = pp.PreprocessingANN(al, fl)
    direct = pp.AlignFeatureLayer(n, list(range(5, 75)), ref[5:75], fl.local, align_weights=w, weights_any_size=True)
    assert layer._flags == direct._flags
    for name in ("align_w", "ref_c", "align_idx", "rec"):
        assert torch.equal(getattr(layer, name), getattr(direct, name)), name


@pytest.mark.parametrize("n_atoms", [80, 256])
def test_torch_twin_of_a_weighted_large_layer_equals_the_oracle(n_atoms):
    from colvarsfinder import pp
    from colvarsfinder.export import ScriptableAlignFeature
    traj, _, ref = frames(n_atoms, 6, seed=40 + n_atoms)
    align = sorted(np.random.RandomState(n_atoms).choice(n_atoms, 3 * n_atoms // 4, replace=False).tolist())
    w = weights_for(n_atoms, len(align))
    feats = [("position", tuple(range(0, n_atoms, 7))), ("bond", (0, 1)), ("angle", (1, 2, 3)), ("dihedral", (4, 5, 6, 7))]
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, align_weights=w, weights_any_size=True)
    # (the layer stores w_hat and ref_c in fp32: the twin is compared on those stored tables' own precision)
    got = ScriptableAlignFeature(layer).double()(torch.tensor(traj, dtype=torch.float64)).numpy()
    want = oracle_features(align, ref, feats, w, traj)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6 * np.abs(want).max())
    cols = position_columns(feats)
    assert np.abs(got[:, cols] - oracle_features(align, ref, feats, None, traj)[:, cols]).max() > NOT_IGNORED


def test_route_of_small_frames_and_refusals_need_no_gpu():
    """cvf_align_feature_route is host arithmetic: the library answers without a device."""
    import ctypes as C

    from colvarsfinder import _hip
    lib = _hip.lib()
    keep = np.zeros(64, dtype=np.float32)
    d = _hip.PPDesc()
    d.mode, d.n_coord, d.n_align, d.n_rec, d.d_r = _hip.PP_ALIGN, 30, 10, 10, 30
    d.align_idx = d.ref_c = d.rec = keep.ctypes.data
    assert lib.cvf_align_feature_route(C.byref(d), 100, 1, 0, 0, 0) == _hip.K1_ROUTE_SMALL
    d.align_w, d.flags = keep.ctypes.data, _hip.PP_ALIGN_CONTIG
    assert lib.cvf_align_feature_route(C.byref(d), 100, 1, 0, 0, 0) < 0 and b"flags == 0" in lib.cvf_last_error()
    d.flags = 0
    assert lib.cvf_align_feature_route(C.byref(d), 100, 1, 0, 0, 0) == _hip.K1_ROUTE_SMALL
    assert lib.cvf_align_feature_route(C.byref(d), 100, 0, 0, 1, 1) < 0      # no output buffer
    assert lib.cvf_align_feature_route(C.byref(d), 0, 1, 0, 0, 0) < 0        # empty batch
    d.mode = _hip.PP_IDENTITY
    assert lib.cvf_align_feature_route(C.byref(d), 100, 1, 0, 0, 0) < 0
