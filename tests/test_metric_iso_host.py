"""CPU: the aligned-frame form of q = J A J^T g that the 16-frame front kernel runs when the metric is isotropic
(csrc/ef16_front_kernel.hpp, the passes behind stamp 26 with launch bit 9), and the rule that selects it.

With ONE coefficient a_b per atom, R a_b R^T = a_b I, and with f_b the atom's feature (its aligned position), r_b its centred
reference position (zero off the align atoms), m_b = 1 on the align atoms:

    pass 1   gbar = sum_b g_b / n_align,   tau = sum_b g_b x f_b,   s = K^-1 tau
    pass 2   G'_b = g_b + m_b (s x r_b - gbar),   u'_b = a_b G'_b,   E = sum_b u'_b . G'_b,
             ubar' = sum_align u'_b / n_align,   om = K^-1 (sum_align r_b x u'_b - rsum x ubar')
    pass 3   q_b = u'_b - ubar' + f_b x om

restated here in fp64 NumPy with the kernel's signs and checked against J A J^T g by autograd through oracle.pp.AlignFeature
(a vector-Jacobian product, the diagonal, a Jacobian-vector product).  Bar: 1e-10 of the largest entry of q - both sides are
fp64 evaluations of the same quantity through an SVD of a well-conditioned 3x3 matrix (make_molecule_traj: sigma = 0.3 around a
reference of scale 2), whose derivative autograd forms with divisions by singular-value gaps of order 1.
"""

import numpy as np
import pytest
import torch

from oracle.pp import AlignFeature, kabsch_frame_np
from tests.synth import diag_coeff_for, make_molecule_traj

BAR = 1e-10


def iso_passes(x, n_rec, n_align, ref_c, g, a_atom):
    """(q [n_rec, 3], E) of one frame by the three aligned-frame passes; x [n_atoms, 3], g [n_rec, 3], a_atom [n_rec]."""
    R, c, Kinv = kabsch_frame_np(x, np.arange(n_align), ref_c)
    f = (x[:n_rec] - c) @ R
    r = np.zeros((n_rec, 3))
    r[:n_align] = ref_c
    m = (np.arange(n_rec) < n_align).astype(np.float64)[:, None]
    gbar = g.sum(axis=0) / n_align
    s = Kinv @ np.cross(g, f).sum(axis=0)
    G = g + m * (np.cross(s[None], r) - gbar)
    u = a_atom[:, None] * G
    E = float((u * G).sum())
    ubar = (m * u).sum(axis=0) / n_align
    om = Kinv @ (np.cross(r, m * u).sum(axis=0) - np.cross(ref_c.sum(axis=0), ubar))
    return u - ubar + np.cross(f, om[None]), E


def oracle_q(x, n_rec, n_align, ref, g, a_coord):
    """J A J^T g and g^T J A J^T g of one frame by autograd; a_coord [3 n_atoms]."""
    torch.set_default_dtype(torch.float64)   # (the layer keeps its reference in the default dtype)
    try:
        layer = AlignFeature(list(range(n_align)), ref[:n_align], [("position", tuple(range(n_rec)))], False)
    finally:
        torch.set_default_dtype(torch.float32)
    xt = torch.tensor(x, dtype=torch.float64)[None]
    gt = torch.tensor(g.reshape(1, -1), dtype=torch.float64)
    _, jtg = torch.autograd.functional.vjp(layer, xt, gt)
    v = torch.tensor(a_coord, dtype=torch.float64).reshape(1, -1, 3) * jtg
    _, q = torch.autograd.functional.jvp(layer, xt, v)
    return q.reshape(n_rec, 3).numpy(), float((q * gt).sum())


# (n_atoms, n_rec, n_align, coefficients): all aligned; a strict prefix; trailing frame atoms that are no features; ones; 1/m
CASES = [("all-aligned", 6, 6, 6, "mass"), ("prefix-3-of-5", 5, 5, 3, "mass"), ("trailing-atoms", 9, 6, 4, "mass"),
         ("ones", 7, 7, 5, "ones"), ("diag-coeff-for", 22, 22, 22, "mass")]


@pytest.mark.parametrize("name,n_atoms,n_rec,n_align,coeff", CASES, ids=[c[0] for c in CASES])
def test_aligned_frame_passes_equal_jajt(name, n_atoms, n_rec, n_align, coeff):
    traj, _, ref = make_molecule_traj(n_atoms, 4, seed=300 + n_atoms + n_align, dtype=np.float64)
    a = np.ones(3 * n_atoms) if coeff == "ones" else diag_coeff_for(n_atoms, 3)
    ref_c = ref[:n_align] - ref[:n_align].mean(axis=0, keepdims=True)
    rs = np.random.RandomState(11)
    for x in traj:
        g = rs.normal(size=(n_rec, 3))
        q, E = iso_passes(x, n_rec, n_align, ref_c, g, a[:3 * n_rec:3])
        qo, Eo = oracle_q(x, n_rec, n_align, ref, g, a)
        scale = np.abs(qo).max()
        print(f"{name}: max |q - q_oracle| / max |q| = {np.abs(q - qo).max() / scale:.2e}, E rel = {abs(E - Eo) / abs(Eo):.2e}")
        assert np.abs(q - qo).max() <= BAR * scale
        assert abs(E - Eo) <= BAR * abs(Eo)


def test_anisotropic_coefficients_break_the_identity():
    """The premise is needed: with one coordinate's coefficient changed the aligned-frame passes no longer give J A J^T g."""
    n = 6
    traj, _, ref = make_molecule_traj(n, 1, seed=5, dtype=np.float64)
    a = diag_coeff_for(n, 3).copy()
    a[4] *= 3.0
    g = np.random.RandomState(2).normal(size=(n, 3))
    q, _ = iso_passes(traj[0], n, n, ref - ref.mean(axis=0, keepdims=True), g, a[::3])
    qo, _ = oracle_q(traj[0], n, n, ref, g, a)
    assert np.abs(q - qo).max() > 1e-3 * np.abs(qo).max()


# ---------------------------------------------------------------------------------------------------- the detection rule
def _rule(a, n_rec):
    from colvarsfinder import core
    return core.metric_is_isotropic(a, n_rec)


def test_rule_isotropic():
    assert _rule(torch.tensor(diag_coeff_for(8, 3), dtype=torch.float32), 8) is True
    assert _rule(torch.ones(24), 8) is True
    assert _rule(torch.tensor(diag_coeff_for(8, 3), dtype=torch.float64), 5) is True


def test_rule_one_ulp_off_is_general():
    a = np.asarray(diag_coeff_for(8, 3), dtype=np.float32)
    n_rec = 6
    for j in range(3):   # each coordinate of the LAST record atom
        b = a.copy()
        b[3 * (n_rec - 1) + j] = np.nextafter(b[3 * (n_rec - 1) + j], np.float32(2.0), dtype=np.float32)
        assert _rule(torch.tensor(b), n_rec) is False, j


def test_rule_ignores_atoms_past_the_record():
    a = np.asarray(diag_coeff_for(8, 3), dtype=np.float32)
    n_rec = 6
    a[3 * n_rec] *= 2.0        # the first coordinate no feature reads
    a[-1] = 0.0
    assert _rule(torch.tensor(a), n_rec) is True
    assert _rule(torch.tensor(a), n_rec + 1) is False


def test_rule_nan_is_general():
    for where in (0, 4, 3 * 6 - 1, 3 * 8 - 1):   # (a NaN past the record too: nothing is assumed about such a vector)
        a = torch.ones(24)
        a[where] = float("nan")
        assert _rule(a, 6) is False, where
    a = torch.ones(24)
    a[3:6] = float("nan")   # a whole atom NaN: NaN != NaN
    assert _rule(a, 6) is False


def test_rule_none_counts_as_ones():
    assert _rule(None, 22) is True


def test_rule_short_vector_is_general():
    assert _rule(torch.ones(9), 4) is False
