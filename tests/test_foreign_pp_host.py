"""CPU: the records of a foreign preprocessing module (colvarsfinder.pp.FactoredMetric) and the checks that refuse what the
generator loss cannot take."""
import numpy as np
import pytest
import torch

from tests.foreign_modules import BatchCentred, Flat3D, PairDistances, Polar, Radius, SmoothContacts
from tests.synth import diag_coeff_for, make_2d_traj, make_molecule_traj


def _fm(module, frames, a):
    from colvarsfinder.pp import FactoredMetric
    return FactoredMetric(module, frames.shape[1:], a, "cpu", frames[:2])


def _check_records(module, frames, a):
    fm = _fm(module, frames, a)
    rec = fm.records(frames).double()
    d_r, rho, n = fm.d_r, fm.rho, fm.n
    assert rec.shape == (frames.shape[0], d_r * (1 + rho))
    X = torch.as_tensor(frames, dtype=torch.float64)
    m64 = fm.module
    for b in range(frames.shape[0]):
        J = torch.autograd.functional.jacobian(lambda x: m64(x[None])[0], X[b]).reshape(d_r, n)
        M = J @ torch.diag(torch.as_tensor(a, dtype=torch.float64) if a is not None else torch.ones(n, dtype=torch.float64)) @ J.T
        # the records are fp32: compare the factor as stored against the fp64 metric, and the fp64 factor itself to 1e-10
        L64 = fm.factor(J[None])[0]
        np.testing.assert_allclose((L64 @ L64.T).numpy(), M.numpy(), rtol=0, atol=1e-10 * max(1.0, float(M.abs().max())))
        L = rec[b, d_r:].reshape(d_r, rho)
        np.testing.assert_allclose((L @ L.T).numpy(), M.numpy(), rtol=0, atol=1e-5 * max(1.0, float(M.abs().max())))
        np.testing.assert_allclose(rec[b, :d_r].numpy(), m64(X[b:b + 1])[0].detach().numpy(), rtol=1e-6, atol=1e-7)
    return fm


def test_records_pair_distances_n_le_dr():
    traj, _, _ = make_molecule_traj(10, 12, seed=3)
    fm = _check_records(PairDistances(10), traj, diag_coeff_for(10, 1))
    assert (fm.d_r, fm.n, fm.rho) == (45, 30, 30)


def test_records_contacts_eigh_branch():
    traj, _, _ = make_molecule_traj(22, 9, seed=4, scale=1.5)
    pairs = [(0, 5), (1, 7), (2, 9), (3, 11), (4, 13), (6, 15), (8, 17), (10, 19), (12, 21), (14, 20), (16, 18), (0, 21)]
    fm = _check_records(SmoothContacts(pairs), traj, diag_coeff_for(22, 2))
    assert (fm.d_r, fm.n, fm.rho) == (12, 66, 12)


def test_records_2d_polar_and_radius():
    traj, _ = make_2d_traj(16, seed=5)
    a = np.array([0.7, 1.9])
    fm = _check_records(Polar(), traj, a)
    assert (fm.d_r, fm.rho) == (3, 2)
    fm = _check_records(Radius(), traj, a)
    assert (fm.d_r, fm.rho) == (1, 1)


def test_records_of_the_oracle_alignment_layer():
    from oracle.pp import AlignFeature
    traj, _, ref = make_molecule_traj(6, 5, seed=6)
    layer = AlignFeature([0, 1, 2, 3], ref[:4], [("position", (0, 1, 2, 3, 4, 5)), ("bond", (0, 4)), ("dihedral", (0, 1, 2, 3))])
    fm = _check_records(layer, traj, diag_coeff_for(6, 3))
    assert (fm.d_r, fm.n, fm.rho) == (21, 18, 18)


def test_users_module_is_not_modified():
    traj, _, _ = make_molecule_traj(10, 4, seed=7)
    m = SmoothContacts([(0, 1), (2, 3)])
    fm = _fm(m, traj, None)
    fm.records(traj)
    assert m.i.dtype == torch.long and fm.dtype == torch.float64
    assert all(p.dtype == torch.float32 for p in m.buffers() if p.is_floating_point())


def test_refusals():
    traj, _, _ = make_molecule_traj(5, 4, seed=8)
    with pytest.raises(ValueError, match="not frame-local"):
        _fm(BatchCentred(), traj, None)
    with pytest.raises(ValueError, match="1-D or 3-D"):
        _fm(Flat3D(), traj, None)
    a = np.ones(15)
    a[3] = -1.0
    with pytest.raises(ValueError, match=">= 0"):
        _fm(PairDistances(5), traj, a)


def test_memory_check_names_the_bytes(monkeypatch):
    """EigenFunctionTask's check against torch.cuda.mem_get_info (called unbound: no device is needed to evaluate it)."""
    from colvarsfinder import core
    task = core.EigenFunctionTask.__new__(core.EigenFunctionTask)
    task.device = torch.device("cuda")
    task.preprocessing_layer = PairDistances(10)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1 << 20, 1 << 30))
    with pytest.raises(NotImplementedError, match=r"4000000 bytes.*lag_tau > 0"):
        task._check_record_memory(4_000_000)
    task._check_record_memory(100_000)   # fits
