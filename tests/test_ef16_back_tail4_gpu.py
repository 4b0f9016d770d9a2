"""GPU (-m gpu): the 4-row and 5-column strips of the 16-frame backward launch (csrc/ef16_back.hip, H = 20) that go to the matrix
cores as 4x4x1 blocks instead of padded 16x16x4 tiles - rows 16 .. 19 of the first layer's column tiles 0 .. 3, and of a hidden
layer's 20 x 21 gradient everything but tile (0, 0) (outer_half44 in csrc/ef_frag.hpp, rows_sum_scatter in csrc/ef16_common.hpp).

(a) One train step (loss_func + backward) against the fp64 oracle, built as tests/test_ef16_back_strip_gpu.py builds it, the route
    asserted to be the 16-frame one.  Position features on the first n_rec atoms, all of them aligned:

      n_rec   D    what it exercises
      5       15   one column tile, CTM = 1
      11      33   the register strip among the first four column tiles
      16      48   the bias column alone
      22      66   the benchmark
      23      69   a ragged fifth tile on the matrix cores
      24      72   `extra` pairs beside the new path

    crossed with the hidden shapes (20,) (no hidden step), (20, 20) (one) and (20, 20, 20) (two, the full tile on another wave in
    each), k in {1, 3}, generator and transfer mode (lag 2), at B = 87: two tiles, the second with one full unit, one part unit and
    two empty waves.  B = 16, 64 and 130 once each at n_rec = 22, hidden (20, 20, 20), k = 3.  Seeds: 7000 + the case's position
    (SEED is empty: no case needed another).  Bars: the sweep's own for its ef16 groups, TOL[("ef16", "gen")] = 6e-6 / 4e-5 / 8e-5
    and TOL[("ef16", "tr")] = 1e-6 / 4e-6 / 8e-6 (loss; npl and eigenvalues; the gradient as a share of its largest entry).
    Worst errors reached on these cases, the parent commit / this tree:

      group                  loss               npl                eigenvalues        gradient / largest entry
      generator (39 cases)   4.1e-7 / 4.1e-7    1.7e-6 / 1.7e-6    1.9e-6 / 1.9e-6    4.9e-6 / 5.0e-6
      transfer  (36 cases)   1.2e-7 / 1.2e-7    1.3e-6 / 1.3e-6    6.3e-7 / 6.3e-7    5.1e-6 / 5.1e-6

    Two cases stand above half a bar, both on the parent already and unchanged by this tree (transfer gradient, bar 8e-6):
    tr-tail4-n16-h20x2-k1-b87 4.11e-6 / 4.11e-6 and tr-tail4-n22-h20x3-k1-b87 5.13e-6 / 5.13e-6.  They keep their seeds.

(b) Reproducibility.  The same step run twice from the same state gives byte-identical flat gradients, and the same bytes again
    after the slab buffer was filled with NaN by an unrelated launch - the slab is not zeroed, so an entry of a block's row that
    nobody wrote would show, and one written twice with different partial sums could not repeat.  D = 66 and D = 72, B = 87 and
    200, both modes.

(c) The MULTI form (a block walks several tiles and accumulates in LDS: `GI[idx] +=` for the new entries) at hidden (20, 20, 20)
    is run by tests/test_ef_sweep_gpu.py in its duplication cases `gen-multi-h20x3` and `tr-multi-h20x3` (n_rec = 6, D = 18,
    B = 33 836 and 17 060, then doubled); `*-multi-h20x1` and `*-multi-h20x2` run the other two H = 20 shapes.  They are not
    repeated here.
"""

import numpy as np
import pytest
import torch

from tests import ef_cases as E
from tests import sweep_errors
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

TOL = {"gen": (6e-6, 4e-5, 8e-5), "tr": (1e-6, 4e-6, 8e-6)}   # TOL[("ef16", mode)] of tests/test_ef_sweep_gpu.py
LAG = 2
N_REC = (5, 11, 16, 22, 23, 24)
HIDDEN = ((20,), (20, 20), (20, 20, 20))
ERRORS = {}


def _cases():
    out = []
    for n_rec in N_REC:
        for hidden in HIDDEN:
            for k in (1, 3):
                for mode in ("gen", "tr"):
                    out.append(E.Case(f"{mode}-tail4-n{n_rec}-h20x{len(hidden)}-k{k}-b87", mode, n_rec, n_rec, n_rec, "pos",
                                      hidden, k, 87, False, False))
    for B in (16, 64, 130):
        out.append(E.Case(f"gen-tail4-n22-h20x3-k3-b{B}", "gen", 22, 22, 22, "pos", (20, 20, 20), 3, B, False, False))
    return out


CASES = _cases()
SEED = {}   # case id -> seed of its batch, where the default (7000 + position in CASES) is replaced; see the module docstring


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


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _task(dev, case, seed):
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    gen, k = case.mode == "gen", case.k
    lag = 0 if gen else LAG
    traj, w, ref = make_molecule_traj(case.n_atoms, case.B + lag, seed=seed, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(case.n_align)), ref_pos=ref[:case.n_align], features=[("position", tuple(range(case.n_rec)))])
    layer = pp.AlignFeatureLayer(case.n_atoms, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    dims = [layer.d_r] + list(case.hidden) + [1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(case.n_atoms, 3), dtype=torch.float32) if gen else None
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    n0 = min(64, case.B)
    task = core.EigenFunctionTask(Traj(traj[:n0 + lag], w[:n0 + lag], 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a,
                                  beta=1.2, lag_tau=lag * 0.5, k=k, device=dev, verbose=False, save_model_every_step=0)
    return task, model, traj, w, spec, sd0, a, eig_w, lag


def _step(task, model, X, wt, Xl, wl):
    task._events = {}
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    task.backward()
    torch.cuda.synchronize()
    launched, task._events = set(task._events), None
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec), launched


# ------------------------------------------------------------------------------------------------ (a) against the fp64 oracle
def test_cases_sit_on_the_new_paths():
    assert [3 * n for n in N_REC] == [15, 33, 48, 66, 69, 72]
    assert all(E.route(c) == "ef16" and E.shape(c) in E.EF16_SHAPES and E.shape(c)[0] == 20 for c in CASES)
    assert all(("ef16_back_kernel", *E.shape(c), 0, int(c.mode == "gen")) in E.instances(c) for c in CASES)
    assert len(CASES) == 75 and len({c.id for c in CASES}) == 75


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_step_vs_fp64_oracle(dev, case):
    from colvarsfinder import _hip
    from oracle import losses
    from oracle.pp import AlignFeature
    gen, k, B = case.mode == "gen", case.k, case.B
    task, model, traj, w, spec, sd0, a, eig_w, lag = _task(dev, case, SEED.get(case.id, 7000 + CASES.index(case)))
    assert bool(_hip.lib().cvf_ef16_supported(task._flat.desc, task._pp))
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, wl = (None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
    v, got, cvec, launched = _step(task, model, X, wt, Xl, wl)
    assert task._route.kind == "ef16", task._route
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
    err = dict(loss=_rel(v[0], float(lo.detach())), npl=_rel(v[1], float(no.detach())), eig=_rel(v[3:], eo.detach().numpy()),
               grad=float(np.abs(got - want).max()) / gmax)
    ERRORS[case.id] = err
    print(f"{case.id}: " + "  ".join(f"{q} {e:.2e}" for q, e in err.items()))
    t_loss, t_eig, t_grad = TOL[case.mode]
    assert cvec == list(co)
    np.testing.assert_allclose(v[0], float(lo.detach()), rtol=t_loss)
    np.testing.assert_allclose(v[1], float(no.detach()), rtol=t_eig)
    np.testing.assert_allclose(v[3:], eo.detach().numpy(), rtol=t_eig)
    np.testing.assert_allclose(got, want, rtol=0, atol=t_grad * gmax)


# ------------------------------------------------------------------------------------------------ (b) reproducibility
@pytest.mark.parametrize("mode", ("gen", "tr"))
@pytest.mark.parametrize("B", (87, 200))
@pytest.mark.parametrize("n_rec", (22, 24))
def test_same_bytes_twice_and_over_a_dirty_slab(dev, mode, B, n_rec):
    case = E.Case(f"{mode}-tail4-repro-n{n_rec}-b{B}", mode, n_rec, n_rec, n_rec, "pos", (20, 20, 20), 3, B, False, False)
    task, model, traj, w, spec, sd0, a, eig_w, lag = _task(dev, case, 7300 + B + n_rec)
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, wl = (None, None) if lag == 0 else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
    v1, g1, _, launched = _step(task, model, X, wt, Xl, wl)
    assert task._route.kind == "ef16" and launched == E.launches(case)
    v2, g2, _, _ = _step(task, model, X, wt, Xl, wl)
    ws = task._workspace(B)
    assert ws is task._last[0] and ws.slab.numel() == ws.slab_rows * task._flat.n
    ws.slab.fill_(float("nan"))   # an unrelated launch that dirties every entry of the slab
    torch.cuda.synchronize()
    v3, g3, _, _ = _step(task, model, X, wt, Xl, wl)
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    assert g1.tobytes() == g2.tobytes(), int((g1 != g2).sum())
    assert g1.tobytes() == g3.tobytes(), (int((g1 != g3).sum()), int(np.isnan(g3).sum()))
    assert v1.tobytes() == v2.tobytes() == v3.tobytes()
