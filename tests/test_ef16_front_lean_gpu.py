"""GPU (-m gpu): the addressing of the 16-frame front launch (csrc/ef16_front_kernel.hpp) at the sizes where it can go wrong.

The launch forms its addresses once per wave and per pass - one register and immediate or scalar offsets - where it formed,
clamped and selected them per access ("front launch: index arithmetic off the wave's path"):

  * the k-step loops of layer 0 and of s = W_1 q read rows 4 s + q without a clamp: a row past d_r must be a zero the block
    wrote, and meet a zero weight;
  * the four-lanes-per-frame passes of q = J A J^T g take the lane's atoms p, p + 4, .. from one base per array and pass, only
    the last iteration is clamped at the ragged end;
  * the q tile, y and E leave through buffer stores, the unit's row of batch sums through offsets formed in front of the barrier.

Shapes: d_r = 15, 33, 45, 48, 66, 69, 72 (every residue of 3N mod 4; 72 is S = 18 = SMAX; 15, 33, 45 and 69 leave the last k-step
and the last column tile partly empty; N = 5, 15, 22 and 23 are no multiple of 4 at NIT = 2, 4, 6, 6), each aligned on all atoms and
on a strict prefix; hidden layers (16,), (20, 20, 20) and (32, 32), every (d_r, align set) with one net and with three, eight nets once; 87 frames
(ragged last unit, partly empty last tile), and 16, 64 and 130 frames once.  Every generator case runs with the isotropic and with a
per-coordinate metric, from the coordinates (the solving twins) and from the batch's alignment rows and feature tile (the ROWS
twins); transfer mode at (20, 20, 20).

Each run is one forward + backward of the step against the fp64 oracle at the bars tests/test_ef_sweep_gpu.py holds for these
quantities (TOL[("ef16", "gen")] and TOL[("ef16", "tr")] there), and is repeated over output buffers filled with NaN: the front
launch's outputs (y, E, the q tile, the hand-off rows, the units' rows of batch sums, the feature tile), the loss vector and the
gradient must come out with the same bytes - nothing may depend on what a buffer held before the launch.
"""

import collections
import gc

import numpy as np
import pytest
import torch

from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

TOL = {"gen": (6e-6, 4e-5, 8e-5), "tr": (1e-6, 4e-6, 8e-6)}   # tests/test_ef_sweep_gpu.py: loss, npl and eigenvalues, gradient / largest
LAG = 2
Case = collections.namedtuple("Case", "n_rec n_align hidden k B")
H16, H20, H32 = (16,), (20, 20, 20), (32, 32)
GEN = [Case(5, 5, H16, 1, 87), Case(5, 3, H20, 3, 87),
       Case(11, 11, H32, 3, 87), Case(11, 7, H16, 1, 87),
       Case(15, 15, H20, 1, 87), Case(15, 9, H32, 3, 87),
       Case(16, 16, H16, 3, 87), Case(16, 10, H20, 1, 87),
       Case(22, 22, H20, 3, 87), Case(22, 13, H32, 1, 87),
       Case(23, 23, H32, 1, 87), Case(23, 17, H16, 3, 87),
       Case(24, 24, H20, 1, 87), Case(24, 17, H20, 3, 87),
       Case(22, 22, H20, 8, 87),
       # the other k of every (d_r, align set) above, at the same hidden layers
       Case(5, 5, H16, 3, 87), Case(5, 3, H20, 1, 87), Case(11, 11, H32, 1, 87), Case(11, 7, H16, 3, 87),
       Case(15, 15, H20, 3, 87), Case(15, 9, H32, 1, 87), Case(16, 16, H16, 1, 87), Case(16, 10, H20, 3, 87),
       Case(22, 22, H20, 1, 87), Case(22, 13, H32, 3, 87), Case(23, 23, H32, 3, 87), Case(23, 17, H16, 1, 87),
       Case(24, 24, H20, 3, 87), Case(24, 17, H20, 1, 87),
       Case(5, 5, H16, 1, 16), Case(22, 22, H20, 3, 64), Case(24, 17, H32, 3, 130)]
TRANSFER = [Case(5, 3, H20, 1, 87), Case(22, 22, H20, 3, 87), Case(23, 23, H20, 1, 87)]


def _id(c):
    return f"d{3 * c.n_rec}-al{c.n_align}-h{c.hidden[0]}x{len(c.hidden)}-k{c.k}-B{c.B}"


def test_the_cases_cover_what_the_addressing_depends_on():
    assert {3 * c.n_rec for c in GEN} == {15, 33, 45, 48, 66, 69, 72}
    assert {3 * c.n_rec % 4 for c in GEN} == {0, 1, 2, 3}
    for n_rec in {c.n_rec for c in GEN}:
        assert {c.n_align == n_rec for c in GEN if c.n_rec == n_rec} == {True, False}
    assert {(c.n_rec + 3) // 4 for c in GEN if c.n_rec % 4} >= {2, 4, 6}
    for key in {(c.n_rec, c.n_align, c.hidden) for c in GEN if c.B == 87 and c.k != 8}:
        assert {c.k for c in GEN if (c.n_rec, c.n_align, c.hidden) == key and c.B == 87} >= {1, 3}, key
    assert 8 in {c.k for c in GEN} and {c.B for c in GEN} == {87, 16, 64, 130}
    assert all(c.hidden == H20 for c in TRANSFER)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    torch.set_default_dtype(torch.float32)
    gc.collect()
    torch.cuda.synchronize()


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _coefficients(case, metric):
    if metric == "iso":
        return torch.tensor(diag_coeff_for(case.n_rec, 3), dtype=torch.float32)
    rs = np.random.RandomState(9100 + 7 * case.n_rec + case.k)   # a coefficient per coordinate, each drawn on its own
    return torch.tensor(rs.choice([1.0, 1.0 / 12.0, 1.0 / 14.0, 1.0 / 16.0], size=3 * case.n_rec), dtype=torch.float32)


def _task(dev, case, a, lag):
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    traj, w, ref = make_molecule_traj(case.n_rec, case.B + lag, seed=7300 + 31 * case.n_rec + case.k + case.B, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(case.n_align)), ref_pos=ref[:case.n_align], features=[("position", tuple(range(case.n_rec)))])
    layer = pp.AlignFeatureLayer(case.n_rec, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    dims = [3 * case.n_rec] + list(case.hidden) + [1]
    sd0 = nnref.init_eigenfunctions(dims, case.k, torch.Generator().manual_seed(17 + case.k))
    model = nn.EigenFunctions(dims, case.k)
    model.load_state_dict(sd0)
    eig_w = [1.0 - 0.1 * i for i in range(case.k)]
    n0 = min(64, case.B) + lag
    task = core.EigenFunctionTask(Traj(traj[:n0], w[:n0], 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2,
                                  lag_tau=lag * 0.5, k=case.k, device=dev, verbose=False, save_model_every_step=0)
    assert task._route.kind == "ef16", task._route
    return task, model, traj, w, spec, sd0, eig_w


def _oracle(case, a, traj, w, spec, sd0, eig_w, names, lag):
    from oracle import losses
    from oracle.pp import AlignFeature
    B = case.B
    torch.set_default_dtype(torch.float64)
    try:
        sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
        ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
        if lag == 0:
            Xo = torch.tensor(traj[:B], dtype=torch.float64, requires_grad=True)
            lo, eo, no, po, co = losses.ef_loss(sd, case.k, ol, Xo, torch.tensor(w[:B]).double(), alpha=12.0, eig_w=eig_w,
                                                diag_coeff=a.double(), beta=1.2)
        else:
            lo, eo, no, po, co = losses.ef_loss(sd, case.k, ol, torch.tensor(traj[:B]).double(), torch.tensor(w[:B]).double(),
                                                torch.tensor(traj[lag:lag + B]).double(), torch.tensor(w[lag:lag + B]).double(),
                                                alpha=12.0, eig_w=eig_w, lag_idx=lag, dt=0.5)
        lo.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n in names]).numpy()
    return float(lo.detach()), float(no.detach()), eo.detach().numpy(), want, list(co)


def _front_outputs(task, ws, lag, rows):
    """What the front launch writes, every element of it: (name, tensor) views."""
    from colvarsfinder import _hip
    lib = _hip.lib()
    n_rows = int(lib.cvf_ef_nstats(task.k, lag)) * int(ws.unit_rows)
    out = [("y", ws.y), ("unit rows of batch sums", ws.scratch[:n_rows])]
    if lag == 0:
        out += [("E", ws.e), ("q tile", ws.q), ("hand-off rows", ws.saved)]
    if not rows:
        out.append(("feature tile", ws._feat[0]))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _run(task, model, ws_args, lag, rows, poison):
    """One forward + backward; with `poison` over outputs filled with NaN.  -> (loss vector, gradient in parameter order, outputs)."""
    X, w, Xl, wl = ws_args
    ws = task._workspace(X.shape[0])
    if poison:
        for _, t in _front_outputs(task, ws, lag, rows):
            t.fill_(float("nan"))
        ws.loss_vec.fill_(float("nan"))
        task._flat.grad.fill_(float("nan"))
    ws = task._forward(X, w, Xl, wl, cache=rows)
    assert (ws.tile is not None) == rows and ws.unit_rows > 0
    task._last = (ws, w, wl)
    task.backward()
    torch.cuda.synchronize()
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    outs = [(n, _bits(t).clone()) for n, t in _front_outputs(task, ws, lag, rows)]
    outs += [("loss vector", _bits(ws.loss_vec).clone()), ("gradient", _bits(task._flat.grad).clone())]
    return ws.loss_vec.cpu().numpy().copy(), g, outs


def _check(case, mode, what, v, g, orc):
    lo, no, eo, want, co = orc
    k = case.k
    err = dict(loss=_rel(v[0], lo), npl=_rel(v[1], no), eig=_rel(v[3:3 + k], eo), grad=float(np.abs(g - want).max() / np.abs(want).max()))
    print(f"{_id(case)} {what}: " + "  ".join(f"{q} {e:.2e}" for q, e in err.items()))
    t_loss, t_eig, t_grad = TOL[mode]
    assert list(np.rint(v[3 + k:3 + 2 * k]).astype(int)) == co
    assert err["loss"] <= t_loss and err["npl"] <= t_eig and err["eig"] <= t_eig and err["grad"] <= t_grad, (what, err, TOL[mode])


def _same_bytes(what, first, second):
    for (name, a), (_, b) in zip(first, second):
        assert torch.equal(a, b), (what, name, int((a != b).sum()), a.numel())


@pytest.mark.parametrize("metric", ["iso", "coord"])
@pytest.mark.parametrize("case", GEN, ids=[_id(c) for c in GEN])
def test_generator_step_from_coordinates_and_from_rows(dev, case, metric):
    a = _coefficients(case, metric)
    task, model, traj, w, spec, sd0, eig_w = _task(dev, case, a, 0)
    assert task.metric_isotropic is (metric == "iso")
    names = [n for n, _ in model.named_parameters()]
    orc = _oracle(case, a, traj, w, spec, sd0, eig_w, names, 0)
    args = (task._dev(torch.tensor(traj[:case.B])), task._dev(torch.tensor(w[:case.B])), None, None)
    for rows in (False, True):
        what = f"{metric}, {'rows' if rows else 'coordinates'}"
        v, g, first = _run(task, model, args, 0, rows, poison=False)
        _check(case, "gen", what, v, g, orc)
        v2, g2, second = _run(task, model, args, 0, rows, poison=True)
        _same_bytes(what, first, second)
    assert task.alignment_fills == 1


@pytest.mark.parametrize("case", TRANSFER, ids=[_id(c) for c in TRANSFER])
def test_transfer_step(dev, case):
    task, model, traj, w, spec, sd0, eig_w = _task(dev, case, None, LAG)
    names = [n for n, _ in model.named_parameters()]
    orc = _oracle(case, None, traj, w, spec, sd0, eig_w, names, LAG)
    B = case.B
    args = tuple(task._dev(torch.tensor(t)) for t in (traj[:B], w[:B], traj[LAG:LAG + B], w[LAG:LAG + B]))
    v, g, first = _run(task, model, args, LAG, False, poison=False)
    _check(case, "tr", "transfer", v, g, orc)
    v2, g2, second = _run(task, model, args, LAG, False, poison=True)
    _same_bytes("transfer", first, second)
