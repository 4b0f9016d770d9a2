"""GPU (-m gpu): one EigenFunctionTask step (loss_func + backward) per case of tests/ef_cases.py against the fp64 oracle - every
compiled instance of the step's kernels (tests/test_ef_instances.py checks that the cases claim them all).

Each case asserts the route the host took (the task's route record and C-ABI launches, and cvf_ef16_supported for the fast
layout), so a shape that silently fell back to another kernel cannot pass as coverage.  The MULTI backward instances (more than
1024 backward tiles) are checked by duplication: two copies of a case's batch give its loss, eigenvalues and gradient, with the
bars of test_gpu_parity.py::test_large_batch_paths_by_duplication; the case itself is checked against the oracle first.

Bars.  The sweep started from KAT_TOL["f64"] of test_gpu_parity.py (1e-6 / 1e-6 / 1e-5), which the golden fixtures meet on
well-conditioned batches of 1000+ frames; on these random nets and small ragged batches (down to 5 frames for 8 nets) the fp32
step lands further from the exact answer, by amounts that follow the batch's conditioning and not the kernel instance.  Each
group's bars are about THREE TIMES its worst achieved error against the fp64 oracle (relative errors; the gradient's as a share
of its largest entry); a MULTI row covers the half batch and the doubled one:

  group (route, mode)                cases   loss      bar      npl / eig   bar      gradient   bar
  ef16 generator (16 x NIT x ALLAL)  192     2.1e-6    6e-6     1.4e-5      4e-5     2.6e-5     8e-5
  ef16 transfer                      16      3.4e-7    1e-6     1.4e-6      4e-6     2.5e-6     8e-6
  ef16 MULTI generator               16      5.7e-8    2e-7     3.2e-7      1e-6     5.3e-7     1.6e-6
  ef16 MULTI transfer                16      5.2e-8    1.6e-7   1.8e-7      6e-7     6.6e-6     2e-5
  fused 64-frame generator           20      3.0e-7    1e-6     3.5e-6      1e-5     1.4e-5     4e-5
  fused 64-frame transfer            20      1.9e-7    6e-7     2.3e-6      7e-6     9.6e-6     3e-5
  plain 64-frame generator (mixed)   24      4.7e-6    1.5e-5   1.4e-5      4e-5     1.6e-5     5e-5
  plain 64-frame transfer (mixed)    24      6.1e-7    2e-6     7.3e-6      2e-5     1.6e-5     5e-5

The duplication identity: the loss rows of the doubled batch equal the half batch's bit for bit in every MULTI case (bar 2e-6);
the gradient entries within rtol 1e-4, atol 2e-6 of the largest.  Left out of that comparison are the nets' output biases,
whose exact gradient is 0 (the loss does not change when a constant is added to an eigenfunction): they hold only the roundoff
of a cancelling sum over the batch, which differs with the summation order (2.9e-6 of the largest entry at k = 1 in transfer
mode); the comparison of both batches with the oracle bounds them.
"""

import numpy as np
import pytest
import torch

from tests import ef_cases as E
from tests import sweep_errors
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

# (group, mode) -> bars for (loss, npl and eigenvalues, gradient / largest entry): the table above
TOL = {("ef16", "gen"): (6e-6, 4e-5, 8e-5), ("ef16", "tr"): (1e-6, 4e-6, 8e-6),
       ("multi", "gen"): (2e-7, 1e-6, 1.6e-6), ("multi", "tr"): (1.6e-7, 6e-7, 2e-5),
       ("fused", "gen"): (1e-6, 1e-5, 4e-5), ("fused", "tr"): (6e-7, 7e-6, 3e-5),
       ("mixed", "gen"): (1.5e-5, 4e-5, 5e-5), ("mixed", "tr"): (2e-6, 2e-5, 5e-5)}
DUP_TOL = dict(rows=2e-6, grad=1e-4, grad_abs=2e-6)   # test_gpu_parity.py::test_large_batch_paths_by_duplication
LAG = 2
ERRORS = {}   # case id -> {quantity: error}; written to $CVF_SWEEP_ERRORS when set


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    sweep_errors.write(ERRORS)


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _spec(case, ref):
    if case.layout == "mixed":
        return dict(align_idx=list(range(case.n_atoms)), ref_pos=ref, features=E.MIXED, use_angle_value=False)
    return dict(align_idx=list(range(case.n_align)), ref_pos=ref[:case.n_align],
                features=[("position", tuple(range(case.n_rec)))], use_angle_value=False)


def _note(case, **errs):
    ERRORS.setdefault(case.id, {}).update({q: float(v) for q, v in errs.items()})


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_step_vs_fp64_oracle(dev, case, monkeypatch):
    from colvarsfinder import _hip, core, nn, pp
    from oracle import losses, nnref
    from oracle.pp import AlignFeature
    if case.no_ef16:
        monkeypatch.setenv("CVF_NO_EF16", "1")
    gen, k, B = case.mode == "gen", case.k, case.B
    lag = 0 if gen else LAG
    traj, w, ref = make_molecule_traj(case.n_atoms, B + lag, seed=6000 + E.CASES.index(case), scale=2.0, sigma=0.3)
    spec = _spec(case, ref)
    layer = pp.AlignFeatureLayer(case.n_atoms, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    dims = [layer.d_r] + list(case.hidden) + [1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(case.n_atoms, 3), dtype=torch.float32) if gen else None
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    task = core.EigenFunctionTask(Traj(traj[:64 + lag], w[:64 + lag], 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a,
                                  beta=1.2, lag_tau=lag * 0.5, k=k, device=dev, verbose=False, save_model_every_step=0)
    assert bool(_hip.lib().cvf_ef16_supported(task._flat.desc, task._pp)) == (E.route(case) == "ef16")
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, wl = (None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))

    def step(n):
        task._events = {}
        cat = (lambda t: t) if n == 1 else (lambda t: None if t is None else torch.cat([t] * n))
        loss, eig, npl, pen, cvec = task.loss_func(cat(X), cat(wt), cat(Xl), cat(wl))
        task.backward()
        torch.cuda.synchronize()
        launched, task._events = set(task._events), None
        g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
        return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec), launched

    v, got, cvec, launched = step(1)
    assert task._route.kind == E.route(case), (task._route, E.route(case))   # the host's own record of the route it took
    assert launched == E.launches(case), (launched, E.launches(case))

    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
    if gen:
        Xo = torch.tensor(traj[:B], dtype=torch.float64, requires_grad=True)
        lo, eo, no, po, co = losses.ef_loss(sd, k, ol, Xo, wt.double(), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(), beta=1.2)
    else:
        lo, eo, no, po, co = losses.ef_loss(sd, k, ol, X.double(), wt.double(), Xl.double(), wl.double(), alpha=12.0, eig_w=eig_w,
                                            lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    gmax = float(np.abs(want).max())
    e_loss, e_npl = _rel(v[0], float(lo.detach())), _rel(v[1], float(no.detach()))
    e_eig, e_grad = _rel(v[3:], eo.detach().numpy()), float(np.abs(got - want).max()) / gmax
    _note(case, loss=e_loss, npl=e_npl, eig=e_eig, grad=e_grad)
    t_loss, t_eig, t_grad = TOL[case.id.split("-")[1], case.mode]

    def check(v, got):
        np.testing.assert_allclose(v[0], float(lo.detach()), rtol=t_loss)
        np.testing.assert_allclose(v[1], float(no.detach()), rtol=t_eig)
        np.testing.assert_allclose(v[3:], eo.detach().numpy(), rtol=t_eig)
        np.testing.assert_allclose(got, want, rtol=0, atol=t_grad * gmax)

    assert cvec == list(co)
    check(v, got)

    if case.dup:   # the MULTI backward instance: every batch sum doubles, the loss is a ratio of sums
        v2, got2, cvec2, launched2 = step(2)
        assert launched2 == launched and cvec2 == cvec
        assert E.instances(case, 2 * B) != E.instances(case)
        _note(case, dup_loss=_rel(v2[0], float(lo.detach())), dup_eig=max(_rel(v2[1], float(no.detach())), _rel(v2[3:], eo.detach().numpy())),
              dup_grad=float(np.abs(got2 - want).max()) / gmax)
        check(v2, got2)
        np.testing.assert_allclose(v2, v, rtol=DUP_TOL["rows"])
        # the output bias of each net (the last parameter of eigen_funcs.<i>): exact gradient 0, see the module docstring
        names = [n for n, _ in model.named_parameters()]
        zero = np.zeros(len(got), dtype=bool)
        pos = np.cumsum([0] + [p.numel() for p in model.parameters()])
        for n in {n.split(".")[1]: n for n in names}.values():
            i = names.index(n)
            assert n.endswith("bias") and pos[i + 1] - pos[i] == 1, n
            zero[pos[i]] = True
        assert np.abs(want[zero]).max() <= 1e-9 * gmax
        np.testing.assert_allclose(got2[~zero], got[~zero], rtol=DUP_TOL["grad"], atol=DUP_TOL["grad_abs"] * np.abs(got).max())
