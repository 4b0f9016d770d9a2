"""Shared inputs of the tests of per-atom alignment weights on frames of more than 64 atoms (``weights_any_size=True``;
csrc/k1_large.hip, the large-frame kernels of k1_vjp.hip and metric_large.hip).

Frames: ``make_molecule_traj(n, B, seed, scale=6.0, sigma=0.4)``; weights: ``RandomState(n).uniform(0.2, 3.0)`` over the align
atoms.  On these inputs the oracle's weighted and unweighted position features differ by 0.08 (5000 atoms) to 0.7 (70 atoms), so
"the weights are not ignored" is asserted as ``> 1e-2`` against the unweighted oracle."""
import numpy as np
import torch

from tests.synth import make_molecule_traj

SCALE, SIGMA = 6.0, 0.4
NOT_IGNORED = 1e-2


def weights_for(n_atoms, n_align):
    return np.random.RandomState(n_atoms).uniform(0.2, 3.0, size=n_align)


def frames(n_atoms, B, seed):
    """(traj [B, N, 3] fp32, frame weights [B], ref [N, 3])"""
    return make_molecule_traj(n_atoms, B, seed, scale=SCALE, sigma=SIGMA)


def position_bond_features(n_atoms, n_pos, n_bond, seed):
    rs = np.random.RandomState(seed)
    feats = [("position", tuple(sorted(int(i) for i in rs.choice(n_atoms, n_pos, replace=False))))]
    return feats + [("bond", tuple(int(i) for i in rs.choice(n_atoms, 2, replace=False))) for _ in range(n_bond)]


def weighted_layer(n_atoms, align, ref, feats, w, dev=None, angle_value=False):
    from colvarsfinder import pp
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, angle_value, align_weights=w, weights_any_size=True)
    return layer if dev is None else layer.to(dev)


def oracle_layer(align, ref, feats, w, angle_value=False):
    """The fp64 oracle (call under torch.set_default_dtype(torch.float64)); w = None: the unweighted layer."""
    from oracle.pp import AlignFeature
    return AlignFeature(align, ref[align], feats, angle_value, align_weights=w)


def oracle_features(align, ref, feats, w, traj, angle_value=False):
    torch.set_default_dtype(torch.float64)
    try:
        return oracle_layer(align, ref, feats, w, angle_value)(torch.tensor(np.asarray(traj), dtype=torch.float64)).numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def position_columns(feats, angle_value=False):
    """Output columns that hold aligned positions (the only features that see the alignment)."""
    cols, out = [], 0
    for t, atoms in feats:
        n = 3 * len(atoms) if t == "position" else (2 if t == "dihedral" and not angle_value else 1)
        if t == "position":
            cols += list(range(out, out + n))
        out += n
    return cols
