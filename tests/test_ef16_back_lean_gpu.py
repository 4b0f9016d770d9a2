"""GPU (-m gpu): the addressing of the 16-frame backward launch (csrc/ef16_back.hip) after its uniform values left the wave's path
(DESIGN 4.1): the nets' offsets come from a per-net base and the compile-time (H, NH) instead of the descriptor's tables, a lane's
four entries of a gradient tile are stored from ONE offset and ONE stride, and the block's coefficients arrive in one go.  No
arithmetic moved, so the values are the parent's; what can go wrong is where they land and whether every entry is written.

(a) One train step against the fp64 oracle, built as tests/test_ef16_back_tail4_gpu.py builds it, the route asserted to be the
    16-frame one.  Position features on the first n_rec atoms, all of them aligned:

      n_rec   D    (D + 1) mod 16   what it exercises
      5       15   0                no ragged tile (one column tile, the bias its last column)
      11      33   2                a strip of 2 columns
      16      48   1                a strip of 1 column: the bias alone
      22      66   3                a strip of 3 columns (the benchmark)
      23      69   6                a ragged fifth tile on the matrix cores
      24      72   9                a column tile beyond the fourth whose rows are dealt out as pairs

    crossed with the hidden shapes (16,) (one full row tile), (20,) and (20, 20, 20) (the 4-row tails; role rotation over two
    hidden steps) and (32, 32) (two full row tiles, tiles dealt round robin), k in {1, 3}, generator and transfer mode (lag 2), at
    B = 87: two tiles, the second with one full unit, one part unit and two empty waves.  B = 16, 64 and 130 once each at
    n_rec = 22, hidden (20, 20, 20), k = 3.  Bars: the sweep's own for its ef16 groups, TOL[("ef16", "gen")] = 6e-6 / 4e-5 / 8e-5 and
    TOL[("ef16", "tr")] = 1e-6 / 4e-6 / 8e-6 of tests/test_ef_sweep_gpu.py (loss; npl and eigenvalues; the gradient as a share of
    its largest entry).  Seeds: the H = 20 cases are the cases of tests/test_ef16_back_tail4_gpu.py with their seeds (7000 + the
    position there), the others 7600 + the position here; chosen before the first run, none replaced.  Worst errors reached:
    generator (51 cases) 4.1e-7 / 1.7e-6 / 1.9e-6 / 5.0e-6 (loss / npl / eigenvalues / gradient), transfer (48 cases) 1.2e-7 / 1.3e-6 /
    6.1e-7 / 5.1e-6 - the H = 20 cases carry the figures they have in the tail4 file, since no arithmetic moved.

(b) In every case the same step is run again, and once more after the slab was filled with NaN: the three flat gradients and loss
    rows are the same bytes.  The slab is not zeroed, so an entry of a block's row that nobody wrote would show as NaN, and an
    entry written twice with different partial sums could not repeat.

(c) The MULTI form (a block walks several tiles and accumulates in LDS; its uniform values are derived again per tile) once per
    H = 20 depth: the sweep's own duplication cases `gen-multi-h20x1`, `tr-multi-h20x2` and `gen-multi-h20x3` with the sweep's seeds
    and bars (TOL[("multi", mode)], DUP_TOL), the doubled batch also run twice and over a NaN slab.

A net layout that is not the regular one (per layer the weight, then the bias, layer after layer) has no second path in the
kernel: the host refuses it, see tests/test_ef16_back_lean_host.py.
"""

import numpy as np
import pytest
import torch

from tests import ef_cases as E
from tests import sweep_errors
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

TOL = {"gen": (6e-6, 4e-5, 8e-5), "tr": (1e-6, 4e-6, 8e-6)}             # TOL[("ef16", mode)] of tests/test_ef_sweep_gpu.py
TOL_MULTI = {"gen": (2e-7, 1e-6, 1.6e-6), "tr": (1.6e-7, 6e-7, 2e-5)}   # TOL[("multi", mode)]
DUP_TOL = dict(rows=2e-6, grad=1e-4, grad_abs=2e-6)                      # DUP_TOL
LAG = 2
N_REC = (5, 11, 16, 22, 23, 24)
HIDDEN = ((16,), (20,), (20, 20, 20), (32, 32))
TAIL4_HIDDEN = ((20,), (20, 20), (20, 20, 20))   # tests/test_ef16_back_tail4_gpu.py: HIDDEN, for the seeds
ERRORS = {}


def _cases():
    out, seeds = [], {}
    for ni, n_rec in enumerate(N_REC):
        for hidden in HIDDEN:
            for ki, k in enumerate((1, 3)):
                for mi, mode in enumerate(("gen", "tr")):
                    c = E.Case(f"{mode}-lean-n{n_rec}-h{hidden[0]}x{len(hidden)}-k{k}-b87", mode, n_rec, n_rec, n_rec, "pos",
                               hidden, k, 87, False, False)
                    if hidden in TAIL4_HIDDEN:
                        seeds[c.id] = 7000 + ((ni * len(TAIL4_HIDDEN) + TAIL4_HIDDEN.index(hidden)) * 2 + ki) * 2 + mi
                    else:
                        seeds[c.id] = 7600 + len(out)
                    out.append(c)
    for j, B in enumerate((16, 64, 130)):
        c = E.Case(f"gen-lean-n22-h20x3-k3-b{B}", "gen", 22, 22, 22, "pos", (20, 20, 20), 3, B, False, False)
        seeds[c.id] = 7000 + len(N_REC) * len(TAIL4_HIDDEN) * 4 + j
        out.append(c)
    return out, seeds


CASES, SEED = _cases()
MULTI_IDS = ("gen-multi-h20x1", "tr-multi-h20x2", "gen-multi-h20x3")
MULTI = [c for c in E.CASES if c.id in MULTI_IDS]


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


def _oracle(case, model, traj, w, spec, sd0, a, eig_w, lag):
    """(loss, eigenvalues, npl, coefficient vector, flat gradient) of the fp64 oracle on the case's batch."""
    from oracle import losses
    from oracle.pp import AlignFeature
    gen, k, B = case.mode == "gen", case.k, case.B
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
    wt = torch.tensor(w[:B]).double()
    if gen:
        Xo = torch.tensor(traj[:B], dtype=torch.float64, requires_grad=True)
        lo, eo, no, po, co = losses.ef_loss(sd, k, ol, Xo, wt, alpha=12.0, eig_w=eig_w, diag_coeff=a.double(), beta=1.2)
    else:
        lo, eo, no, po, co = losses.ef_loss(sd, k, ol, torch.tensor(traj[:B]).double(), wt, torch.tensor(traj[lag:lag + B]).double(),
                                            torch.tensor(w[lag:lag + B]).double(), alpha=12.0, eig_w=eig_w, lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    return float(lo.detach()), eo.detach().numpy(), float(no.detach()), list(co), want


def _check(v, got, oracle, tol):
    lo, eo, no, _, want = oracle
    t_loss, t_eig, t_grad = tol
    np.testing.assert_allclose(v[0], lo, rtol=t_loss)
    np.testing.assert_allclose(v[1], no, rtol=t_eig)
    np.testing.assert_allclose(v[3:], eo, rtol=t_eig)
    np.testing.assert_allclose(got, want, rtol=0, atol=t_grad * float(np.abs(want).max()))


def _same_bytes_again_and_over_a_dirty_slab(task, model, batch, v1, g1, n_frames):
    v2, g2, _, _ = _step(task, model, *batch)
    ws = task._workspace(n_frames)
    assert ws is task._last[0] and ws.slab.numel() == ws.slab_rows * task._flat.n
    ws.slab.fill_(float("nan"))   # an unrelated launch that dirties every entry of the slab
    torch.cuda.synchronize()
    v3, g3, _, _ = _step(task, model, *batch)
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    assert g1.tobytes() == g2.tobytes(), int((g1 != g2).sum())
    assert g1.tobytes() == g3.tobytes(), (int((g1 != g3).sum()), int(np.isnan(g3).sum()))
    assert v1.tobytes() == v2.tobytes() == v3.tobytes()


def test_cases_cover_the_addressing():
    assert [3 * n for n in N_REC] == [15, 33, 48, 66, 69, 72] and [(3 * n + 1) % 16 for n in N_REC] == [0, 2, 1, 3, 6, 9]
    assert len(CASES) == 6 * 4 * 2 * 2 + 3 and len({c.id for c in CASES}) == len(CASES) and len(set(SEED.values())) == len(CASES)
    assert all(E.route(c) == "ef16" and E.shape(c) in E.EF16_SHAPES for c in CASES)
    assert all(("ef16_back_kernel", *E.shape(c), 0, int(c.mode == "gen")) in E.instances(c) for c in CASES)
    assert [c.id for c in MULTI] == list(MULTI_IDS) and all(c.dup for c in MULTI)
    assert all(("ef16_back_kernel", *E.shape(c), 1, int(c.mode == "gen")) in E.instances(c, 2 * c.B) for c in MULTI)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_step_vs_fp64_oracle_and_same_bytes(dev, case):
    from colvarsfinder import _hip
    gen, B = case.mode == "gen", case.B
    task, model, traj, w, spec, sd0, a, eig_w, lag = _task(dev, case, SEED[case.id])
    assert bool(_hip.lib().cvf_ef16_supported(task._flat.desc, task._pp))
    batch = (torch.tensor(traj[:B]), torch.tensor(w[:B])) + ((None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B])))
    v, got, cvec, launched = _step(task, model, *batch)
    assert task._route.kind == "ef16", task._route
    assert launched == E.launches(case), (launched, E.launches(case))
    oracle = _oracle(case, model, traj, w, spec, sd0, a, eig_w, lag)
    lo, eo, no, co, want = oracle
    err = dict(loss=_rel(v[0], lo), npl=_rel(v[1], no), eig=_rel(v[3:], eo), grad=float(np.abs(got - want).max()) / float(np.abs(want).max()))
    ERRORS[case.id] = err
    print(f"{case.id}: " + "  ".join(f"{q} {e:.2e}" for q, e in err.items()))
    assert cvec == co
    _check(v, got, oracle, TOL[case.mode])
    _same_bytes_again_and_over_a_dirty_slab(task, model, batch, v, got, B)


@pytest.mark.parametrize("case", MULTI, ids=[c.id for c in MULTI])
def test_multi_form_by_duplication(dev, case):
    """As tests/test_ef_sweep_gpu.py runs its duplication cases (same batch: seed 6000 + the case's position in the sweep)."""
    gen, B = case.mode == "gen", case.B
    task, model, traj, w, spec, sd0, a, eig_w, lag = _task(dev, case, 6000 + E.CASES.index(case))
    half = (torch.tensor(traj[:B]), torch.tensor(w[:B])) + ((None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B])))
    twice = tuple(None if t is None else torch.cat([t, t]) for t in half)
    v, got, cvec, launched = _step(task, model, *half)
    assert task._route.kind == "ef16" and launched == E.launches(case)
    oracle = _oracle(case, model, traj, w, spec, sd0, a, eig_w, lag)
    lo, eo, no, co, want = oracle
    assert cvec == co
    _check(v, got, oracle, TOL_MULTI[case.mode])
    v2, got2, cvec2, launched2 = _step(task, model, *twice)   # more than 1024 backward tiles: the MULTI instance
    assert launched2 == launched and cvec2 == cvec and E.instances(case, 2 * B) != E.instances(case)
    err = dict(loss=_rel(v2[0], lo), npl=_rel(v2[1], no), eig=_rel(v2[3:], eo), grad=float(np.abs(got2 - want).max()) / float(np.abs(want).max()))
    ERRORS[case.id + "-lean"] = err
    print(f"{case.id} doubled: " + "  ".join(f"{q} {e:.2e}" for q, e in err.items()))
    _check(v2, got2, oracle, TOL_MULTI[case.mode])
    np.testing.assert_allclose(v2, v, rtol=DUP_TOL["rows"])
    # the output bias of each net (the last parameter of eigen_funcs.<i>): exact gradient 0, only the roundoff of a cancelling sum
    sizes = [p.numel() for p in model.parameters()]
    per_net = sum(sizes) // case.k
    zero = np.zeros(len(got), dtype=bool)
    zero[[per_net * (i + 1) - 1 for i in range(case.k)]] = True
    assert np.abs(want[zero]).max() <= 1e-9 * float(np.abs(want).max())
    np.testing.assert_allclose(got2[~zero], got[~zero], rtol=DUP_TOL["grad"], atol=DUP_TOL["grad_abs"] * np.abs(got).max())
    _same_bytes_again_and_over_a_dirty_slab(task, model, twice, v2, got2, 2 * B)
