"""GPU (-m gpu): the optimiser at task level.  With optimizer_name other than 'Adam' the tasks take a branch of their own -
_FusedOptimizer.fused_args() is None, so a separate cvf_sgd_step launch follows the gradient; in EigenFunctionTask inside the
captured graphs too (AutoEncoderTask and RegAutoEncoderTask launch every step eagerly).

SGD traces (tests/optim_tasks.py): three epochs of three steps through train() - EigenFunctionTask's graphs replay from the
second epoch - against the fp64 oracle (oracle/train.py, torch.optim.SGD) on the same split: every step's loss row, train and
test, and the final parameters.  SGD is linear in the gradient, so the trace is as well conditioned as the gradient; the bars
(optim_tasks.BARS) are about three times the worst error achieved on an MI355X, none above
test_gpu_parity.TRACE_TOL["f64"] = 1e-5:

  case                            loss rows   bar       final parameters   bar
  ef16-generator                  3.2e-7      1.0e-6    1.0e-7             3.0e-7
  fused-transfer                  3.5e-7      1.0e-6    4.0e-8             1.2e-7
  plain-generator-mixed           2.1e-6      6.0e-6    1.3e-7             4.0e-7
  padded-40-to-48                 5.0e-7      1.5e-6    1.5e-7             4.5e-7
  general-72-33                   1.0e-6      3.0e-6    3.0e-7             9.0e-7
  ae-register-resident            5.3e-8      1.6e-7    8.0e-8             2.4e-7
  ae-mfma                         4.9e-8      1.5e-7    7.2e-8             2.2e-7
  ae-general                      5.3e-8      1.6e-7    5.6e-8             1.7e-7
  regae-frozen-encoder            4.0e-8      1.2e-7    8.9e-8             2.7e-7
  regae-generator-regulariser     8.8e-8      2.6e-7    1.1e-7             3.3e-7

Every case's learning rate moves each trainable tensor of the oracle by at least 100 x the parameter bar
(tests/test_optim_cases.py::test_sgd_cases_move_the_oracle, on the CPU): a missing update cannot pass."""
import gc

import numpy as np
import pytest
import torch

from tests import optim_tasks as O
from tests import sweep_errors
from tests.synth import Traj

pytestmark = pytest.mark.gpu

SWITCHES = ("CVF_NO_EF16", "CVF_NO_EF16_TRANSFER", "CVF_NO_TRANSFER_ROWS", "CVF_NO_ALIGN_FWD", "CVF_PIPELINE", "CVF_NO_FWD_METRIC",
            "CVF_NO_ALIGN_FUSED", "CVF_ALIGN_CACHE", "CVF_NO_AE16", "CVF_GRAPH")
ERRORS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _collect_tasks():
    """A test's tasks are cyclic garbage when it returns (they may hold captured graphs); collected here."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.set_default_dtype(torch.float32)


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    sweep_errors.write(ERRORS)


def build(dev, case, inp, monkeypatch):
    """(task, model) of one case, with optimizer_name as the case spells it."""
    from colvarsfinder import core, nn, pp
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    kw = dict(learning_rate=case.lr, batch_size=O.BATCH, num_epochs=O.EPOCHS, test_ratio=0.2, optimizer_name=case.name, device=dev,
              verbose=False, save_model_every_step=0)
    if case.kind == "ef":
        n_atoms, _, _, k, lag, general = case.spec
        sp, h = inp["spec"], O.EF_HYPER
        layer = pp.AlignFeatureLayer(n_atoms, sp["align_idx"], sp["ref_pos"], sp["features"], sp["use_angle_value"]).to(dev)
        model = nn.EigenFunctions(inp["dims"], k)
        model.load_state_dict(inp["sd0"])
        task = core.EigenFunctionTask(Traj(inp["traj"], inp["w"], h["dt"]), layer, model, "/tmp/cvf_test", h["alpha"], h["eig_w"],
                                      diag_coeff=inp["diag_coeff"], beta=h["beta"], lag_tau=lag * h["dt"], k=k, general_nets=general, **kw)
    elif case.kind == "ae":
        model = nn.AutoEncoder(*case.spec)
        model.load_state_dict(inp["sd0"])
        task = core.AutoEncoderTask(Traj(inp["traj"], inp["w"], 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", **kw)
    else:
        e_dims, d_dims, r_dims, K, lag_reg, frozen = case.spec
        h = O.REGAE_HYPER
        model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K)
        model.load_state_dict(inp["sd0"])
        task = core.RegAutoEncoderTask(Traj(inp["traj"], inp["w"], h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=h["eig_w"],
                                       alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"], lag_tau_ae=h["lag_ae"] * h["dt"],
                                       lag_tau_reg=lag_reg * h["dt"], beta=h["beta"], freeze_encoder=frozen, **kw)
    return task, model


def check_route(case, task):
    from colvarsfinder import _hip
    assert task.optimizer.name == "sgd" and task.optimizer.fused_args() is None
    if case.kind == "ef" and case.route is not None:
        assert task._route.kind == case.route, task._route
    if case.kind == "ae":
        fl = task._flat
        code = _hip.lib().cvf_ae_step_route(fl.desc, _hip.ptr(fl.theta), 1, None)
        assert {"ae16": code == 0, "mfma": code in (1, 2), "general": code < 0 and task._general[True]}[case.route], code


@pytest.mark.parametrize("case", O.CASES, ids=[c.id for c in O.CASES])
def test_sgd_trace_vs_fp64_oracle(dev, case, monkeypatch):
    from colvarsfinder import _hip
    inp = O.inputs(case)
    want = O.oracle_trace(case, inp)
    task, model = build(dev, case, inp, monkeypatch)
    check_route(case, task)
    start = {n: p.detach().cpu().clone() for n, p in model.state_dict().items()}
    fl = task._flat
    real = None
    if case.id.startswith("padded"):
        assert fl._views is not None and fl.desc.dims[1] == 48, "the case is meant to run on the zero-padded layout"
        fl.grad.zero_()
        for _, gv in fl.grad_views():
            gv.fill_(1.0)
        real = fl.grad.clone() == 1.0            # entries of the flat buffer that belong to the nets the user built
        fl.grad.zero_()
        assert 0 < int((~real).sum()) and (fl.theta[~real] == 0).all()
    np.random.seed(O.SEED)
    task.train()
    torch.cuda.synchronize()
    if case.kind == "ef":
        assert task._use_graphs and task._graphs, "the epochs after the first are meant to replay captured graphs"
    tr = np.stack([np.asarray(e[0].numpy(), dtype=np.float64) for e in task.loss_list])
    te = np.stack([np.asarray(e[1].numpy(), dtype=np.float64) for e in task.loss_list])
    final = {n: p.detach().cpu().double().numpy() for n, p in model.state_dict().items()}
    e_rows = max(O.row_error(tr, want["train"]), O.row_error(te, want["test"]))
    e_par = O.param_error(final, want["final"])
    print(f"sgd trace {case.id}: loss rows {e_rows:.2e}  final parameters {e_par:.2e}")
    ERRORS["optimizer_tasks::sgd::" + case.id] = dict(rows=e_rows, params=e_par)
    for n, p in start.items():                  # what must not move did not, bit for bit where nothing touches it
        if case.kind == "regae" and case.spec[5] and n.startswith("encoder."):
            assert torch.equal(model.state_dict()[n].cpu(), p), f"frozen {n} changed"
    if real is not None:
        assert (fl.theta[~real] == 0).all(), "padding entries of theta left 0"
    if getattr(fl, "packed", None) is not None:
        fresh = torch.full_like(fl.packed, -7.25e33)
        _hip.check(_hip.lib().cvf_ef_pack(fl.desc, _hip.ptr(fl.theta), _hip.ptr(fresh), _hip.stream()), "cvf_ef_pack")
        assert torch.equal(fl.packed, fresh), "fragment copy is not the pack of the final parameters"
    bar_rows, bar_par = O.BARS[case.id]
    assert bar_rows <= O.CEILING and bar_par <= O.CEILING
    assert e_rows <= bar_rows and e_par <= bar_par, (e_rows, e_par)


# ------------------------------------------------------------------------------------------------ one step, every shape
def _step_cases():
    """One case of tests/ef_cases.py per (H, NH) and route group - 16-frame generator, 16-frame transfer, fused, plain (the
    64-frame groups alternate between generator and transfer mode) - and the zero-padded, five-layer and D = 200 shapes."""
    from tests import ef_cases as E
    out, seen = [], set()
    for c in E.CASES:
        if c.dup:
            continue
        r = E.route(c)
        group = (r + "-" + c.mode) if r == "ef16" else r
        key = (group, E.shape(c))
        want_mode = ("gen", "tr")[len([k_ for k_ in seen if k_[0] == group]) % 2]
        if key in seen or (r != "ef16" and c.mode != want_mode):
            continue
        seen.add(key)
        out.append(c)
    extra = [E.Case("gen-padded-40-to-48", "gen", 9, 9, 9, "pos", (40, 40), 2, 100, False, False),
             E.Case("tr-padded-10-to-20x5", "tr", 10, 0, 0, "mixed", (20, 16, 12, 10, 10), 2, 100, False, False),
             E.Case("gen-five-layers-32", "gen", 10, 0, 0, "mixed", (32,) * 5, 2, 100, False, False),
             E.Case("gen-d200", "gen", 0, 0, 0, "identity200", (16, 16), 3, 100, False, False)]
    return out + extra


STEP_CASES = _step_cases()
STEP_MODES = ("fused_train_step", "public_step", "sgd_train_step")
LAG = 2


def _step_task(dev, case, optimizer_name, monkeypatch):
    """(task, device arguments of train_step, host arguments of loss_func)."""
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from tests.synth import diag_coeff_for, make_molecule_traj, make_weights
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if case.no_ef16:
        monkeypatch.setenv("CVF_NO_EF16", "1")
    gen, k, B = case.mode == "gen", case.k, case.B
    lag = 0 if gen else LAG
    seed = 7000 + STEP_CASES.index(case)
    if case.layout == "identity200":
        rs = np.random.RandomState(seed)
        traj = (0.4 * rs.normal(size=(B + lag, 200))).astype(np.float64)
        w = make_weights(rs, B + lag)
        layer, d_r = torch.nn.Identity(), 200
        a = torch.tensor(rs.uniform(0.3, 1.5, size=200), dtype=torch.float32) if gen else None
    else:
        traj, w, ref = make_molecule_traj(case.n_atoms, B + lag, seed=seed, scale=2.0, sigma=0.3)
        if case.layout == "mixed":
            al, feats = list(range(case.n_atoms)), O.MIXED
        else:
            al, feats, ref = list(range(case.n_align)), [("position", tuple(range(case.n_rec)))], ref[:case.n_align]
        layer = pp.AlignFeatureLayer(case.n_atoms, al, ref, feats, False).to(dev)
        d_r = layer.d_r
        a = torch.tensor(diag_coeff_for(case.n_atoms, 3), dtype=torch.float32) if gen else None
    dims = [d_r] + list(case.hidden) + [1]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k)))
    task = core.EigenFunctionTask(Traj(traj[:64 + lag], w[:64 + lag], 0.5), layer, model, "/tmp/cvf_test", 12.0,
                                  [1.0 - 0.1 * i for i in range(k)], diag_coeff=a, beta=1.2, lag_tau=lag * 0.5, k=k, device=dev,
                                  learning_rate=1e-3, optimizer_name=optimizer_name, verbose=False, save_model_every_step=0)
    host = [torch.tensor(traj[:B]), torch.tensor(w[:B]), None if gen else torch.tensor(traj[lag:lag + B]),
            None if gen else torch.tensor(w[lag:lag + B])]
    device = [None if t is None else (t.to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous() if i % 2 == 0
                                      else t.to(device=dev, dtype=torch.float32)) for i, t in enumerate(host)]
    return task, device, host


@pytest.mark.parametrize("mode", STEP_MODES)
@pytest.mark.parametrize("case", STEP_CASES, ids=[c.id for c in STEP_CASES])
def test_one_step_updates_parameters_and_fragments(dev, case, mode, monkeypatch):
    """Two optimiser steps; the second (non-zero moments, t = 2) is compared with the fp64 update formula applied to the GPU's
    own flat gradient and the state before it - Adam in the metrics and at the bars of tests/test_optimizer_gpu.py, SGD at
    2^-23 (|th0| + |lr g|).  Then the fragment copy is the pack of the new parameters without any repack inside the step, and the
    kernels give the same loss vector and gradient, bit for bit, from the copy the updater left and from a fresh pack."""
    from colvarsfinder import _hip
    from tests import optim_cases as OC
    from tests.optim_inputs import adam_metrics, torch_adam
    task, device, host = _step_task(dev, case, "SGD" if mode == "sgd_train_step" else "Adam", monkeypatch)
    fl, opt = task._flat, task.optimizer
    assert fl.packed is not None
    repacks, real_repack, live = [0], fl.repack, [True]

    def counting_repack():
        repacks[0] += 1
        if live[0]:
            real_repack()

    fl.repack = counting_repack
    pad = None
    if fl._views is not None:
        fl.grad.zero_()
        for _, gv in fl.grad_views():
            gv.fill_(1.0)
        pad = fl.grad.clone() != 1.0
        fl.grad.zero_()
        assert int(pad.sum()) > 0

    def one_step():
        if mode == "public_step":
            task.loss_func(*host)
            task.backward()
            n0 = repacks[0]
            opt.step()
            return n0
        n0 = repacks[0]
        task.train_step(*device)
        return n0

    one_step()
    torch.cuda.synchronize()
    th0, m0, v0 = (t.detach().cpu().clone() for t in (fl.theta, opt.exp_avg, opt.exp_avg_sq))
    n0 = one_step()
    torch.cuda.synchronize()
    assert repacks[0] == n0, "the step repacked the fragment copy itself"
    th, m, v, g = (t.detach().cpu().clone() for t in (fl.theta, opt.exp_avg, opt.exp_avg_sq, fl.grad))
    assert not torch.equal(th, th0)
    if pad is not None:
        assert (th[pad.cpu()] == 0).all() and (g[pad.cpu()] == 0).all(), "padding entries left 0"
    lr32 = float(np.float32(1e-3))
    if mode == "sgd_train_step":
        th64 = th0.double().numpy() - lr32 * g.double().numpy()
        bound = 2.0 ** -23 * (np.abs(th0.double().numpy()) + np.abs(lr32 * g.double().numpy()))
        err = np.abs(th.double().numpy() - th64)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert int(opt.step_count.item()) in (0, 2)
    else:
        assert int(opt.step_count.item()) == 2
        ref64 = torch_adam(th0, g, m0, v0, 2, lr32, opt.betas, opt.eps, torch.float64)
        ref32 = torch_adam(th0, g, m0, v0, 2, lr32, opt.betas, opt.eps, torch.float32)
        e32 = adam_metrics(ref32, ref64, th0, g, m0, 2, lr32, opt.betas, opt.eps)
        e = adam_metrics([x.numpy() for x in (th, m, v)], ref64, th0, g, m0, 2, lr32, opt.betas, opt.eps)
        for name in ("m", "v", "th"):
            assert e[name] <= max(OC.ADAM_BAR_FACTOR * e32[name], OC.ADAM_BAR_FLOOR), (name, e[name], e32[name])
    fresh = torch.full_like(fl.packed, -7.25e33)
    _hip.check(_hip.lib().cvf_ef_pack(fl.desc, _hip.ptr(fl.theta), _hip.ptr(fresh), _hip.stream()), "cvf_ef_pack")
    assert torch.equal(fl.packed, fresh), "fragment copy is not the pack of the new parameters"
    # the same loss and gradient from the copy the updater left (repack held back) and from a fresh pack
    out = []
    for fresh_pack in (False, True):
        live[0] = fresh_pack
        n0 = repacks[0]
        task.loss_func(*host)
        task.backward()
        torch.cuda.synchronize()
        assert repacks[0] > n0 or not fresh_pack
        out.append((task._last[0].loss_vec.detach().cpu().clone(), fl.grad.detach().cpu().clone()))
    live[0] = True
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
