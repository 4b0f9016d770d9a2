"""Cases, data and fp64 references of EigenFunctionTask on a colvarsfinder.nn.SharedEigenFunctions model (one trunk, k heads), shared
by tests/test_shared_ef_task_host.py (CPU: the eigenvalues of every case are well apart) and tests/test_shared_ef_task_gpu.py.

Reference of a step: oracle.losses.ef_loss in fp64, the trunk's layers passed as the SAME leaf tensors for every net (autograd sums
their gradient).  Reference of train(): an fp64 torch loop written here - oracle.train.split_indices (drawn twice, the second kept),
static batches with the tail dropped, oracle.losses.ef_loss, torch.optim.Adam on the shared leaves, the test pass after the train
pass of every epoch.  Bars: 8 x the distance of the same computation in fp32 on the CPU from the fp64 one.

Frames are AR(1) sequences (one correlation per coordinate / per atom), so that the time-lagged eigenvalues of the nets differ by far
more than the bars.
"""
import functools
import itertools

import numpy as np
import torch

from tests.synth import diag_coeff_for, random_rotations

N_ATOMS, LAG, DT, ALPHA, BETA = 10, 2, 0.5, 12.0, 1.2
B_STEP = 200
MODELS = {"deep": lambda d: ([d, 20, 20], [20, 20, 1]), "wide": lambda d: ([d, 33], [33, 1])}
# (mode, data, k, model): both modes, Identity on 2-D data and a 10-atom AlignFeatureLayer with position features, k = 2 and 3
STEP_CASES = list(itertools.product(("gen", "tr"), ("plane", "mol10"), (2, 3), ("deep", "wide")))
TRAIN_CASES = [("tr", "mol10", 3, "deep"), ("gen", "plane", 2, "wide")]
TRAIN = dict(n_frames=300, batch_size=100, num_epochs=2, learning_rate=2e-3, test_ratio=0.2, seed=41)


def case_id(c):
    return "-".join(str(x) for x in c)


def eig_w(k):
    return [1.0 - 0.1 * i for i in range(k)]


def _ar1(rs, n, shape, rho, sigma):
    x = np.empty((n,) + shape)
    x[0] = sigma * rs.normal(size=shape)
    for t in range(1, n):
        x[t] = rho * x[t - 1] + np.sqrt(1.0 - rho * rho) * sigma * rs.normal(size=shape)
    return x


@functools.lru_cache(maxsize=None)
def frames(data, n, seed):
    """(traj fp32, weights fp64, ref or None): "plane" [n, 2]; "mol10" [n, 10, 3], rotated and shifted copies of ref + AR(1) noise."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.5, 1.5, size=n)
    if data == "plane":
        return _ar1(rs, n, (2,), np.array([0.95, 0.4]), 1.0).astype(np.float32), w, None
    ref = rs.normal(scale=2.0, size=(N_ATOMS, 3))
    xi = _ar1(rs, n, (N_ATOMS, 3), np.linspace(0.3, 0.97, N_ATOMS)[:, None], 0.3)
    x = np.einsum("bij,baj->bai", random_rotations(rs, n), ref[None] + xi) + rs.normal(size=(n, 1, 3))
    return x.astype(np.float32), w, ref


FEATS = [("position", tuple(range(N_ATOMS)))]


def task_layer(data, ref, dev):
    from colvarsfinder import pp
    if data == "plane":
        return torch.nn.Identity()
    return pp.AlignFeatureLayer(N_ATOMS, list(range(N_ATOMS)), ref, FEATS, False).to(dev)


def oracle_layer(data, ref):
    from oracle.pp import AlignFeature
    return (lambda x: x) if data == "plane" else AlignFeature(list(range(N_ATOMS)), ref, FEATS, False)


def d_r(data):
    return 2 if data == "plane" else 3 * N_ATOMS


def diag_coeff(data):
    return torch.tensor([1.0, 0.5] if data == "plane" else diag_coeff_for(N_ATOMS, 3), dtype=torch.float32)


def tie(sd, k, ns):
    """``sd`` with net 0's first ns layers standing in every net (the same tensor objects)."""
    sd = dict(sd)
    for i in range(1, k):
        for l in range(ns):
            for n in ("weight", "bias"):
                sd[f"eigen_funcs.{i}.{l + 1}.{n}"] = sd[f"eigen_funcs.0.{l + 1}.{n}"]
    return sd


@functools.lru_cache(maxsize=None)
def init(data, k, model, seed):
    """(trunk_dims, head_dims, initial state_dict - the keys of the model's, the trunk's tensors under every net)."""
    from oracle import nnref
    trunk, head = MODELS[model](d_r(data))
    sd = nnref.init_eigenfunctions(trunk + head[1:], k, torch.Generator().manual_seed(seed))
    return trunk, head, tie(sd, k, len(trunk) - 1)


def build_model(case, seed):
    from colvarsfinder import nn
    mode, data, k, model = case
    trunk, head, sd0 = init(data, k, model, seed)
    m = nn.SharedEigenFunctions(trunk, head, k)
    m.load_state_dict(sd0)
    return m, sd0


def param_names(case):
    """The model's parameters() order as state_dict names: the trunk (under net 0), then head by head."""
    mode, data, k, model = case
    trunk, head = MODELS[model](d_r(data))
    ns, L = len(trunk) - 1, len(trunk) + len(head) - 2
    names = [f"eigen_funcs.0.{l + 1}.{n}" for l in range(ns) for n in ("weight", "bias")]
    return names + [f"eigen_funcs.{i}.{l + 1}.{n}" for i in range(k) for l in range(ns, L) for n in ("weight", "bias")]


def output_biases(case):
    mode, data, k, model = case
    trunk, head = MODELS[model](d_r(data))
    return {f"eigen_funcs.{i}.{len(trunk) + len(head) - 2}.bias" for i in range(k)}


# seeds of a case's parameters and frames: 9000 + its place in the table, except where that seed's fp64 eigenvalues lie close together
STEP_SEEDS = {("gen", "plane", 2, "deep"): 9109, ("tr", "mol10", 3, "deep"): 9109}
TRAIN_SEED = 9628   # (among ten seeds the one whose eigenvalues stay furthest apart over all steps of both training loops)


def step_seed(case):
    return STEP_SEEDS.get(case, 9000 + STEP_CASES.index(case))


def _loss(sd, case, ol, X, w, Xl, wl, dtype):
    from oracle import losses
    mode, data, k, model = case
    if mode == "gen":
        return losses.ef_loss(sd, k, ol, X.clone().requires_grad_(True), w, alpha=ALPHA, eig_w=eig_w(k), diag_coeff=diag_coeff(data).to(dtype),
                              beta=BETA)
    return losses.ef_loss(sd, k, ol, X, w, Xl, wl, alpha=ALPHA, eig_w=eig_w(k), lag_idx=LAG, dt=DT)


def step_oracle(case, dtype):
    """(loss vector [loss, npl, pen], eigenvalues, cvec, gradient in parameters() order) of one step in ``dtype``."""
    mode, data, k, model = case
    traj, w, ref = frames(data, B_STEP + LAG, step_seed(case))
    trunk, head, sd0 = init(data, k, model, step_seed(case))
    torch.set_default_dtype(dtype)
    try:
        sd = tie({n: p.to(dtype).requires_grad_(True) for n, p in sd0.items()}, k, len(trunk) - 1)
        X, wt = torch.tensor(traj, dtype=dtype), torch.tensor(w, dtype=dtype)
        lo, eo, no, po, co = _loss(sd, case, oracle_layer(data, ref), X[:B_STEP], wt[:B_STEP], X[LAG:], wt[LAG:], dtype)
        lo.backward()
        grad = torch.cat([sd[n].grad.reshape(-1) for n in param_names(case)])
    finally:
        torch.set_default_dtype(torch.float32)
    return (np.asarray([float(lo.detach()), float(no.detach()), float(po.detach())]), eo.double().numpy(), [int(c) for c in co],
            grad.double().numpy())


def errors(got, want):
    """(loss vector, eigenvalues, gradient / its largest entry) distances of a result from the fp64 one."""
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))   # noqa: E731
    return rel(got[0], want[0]), rel(got[1], want[1]), float(np.abs(got[3] - want[3]).max() / np.abs(want[3]).max())


@functools.lru_cache(maxsize=None)
def step_reference():
    """({case: fp64 oracle}, bars) - computed once per process, never modified."""
    ref, worst = {}, [0.0, 0.0, 0.0]
    for case in STEP_CASES:
        ref[case] = want = step_oracle(case, torch.float64)
        worst = [max(a, b) for a, b in zip(worst, errors(step_oracle(case, torch.float32), want))]
    bars = dict(zip(("loss", "eig", "grad"), (8.0 * e for e in worst)))
    print(f"[shared-task] step bars (8 x fp32 CPU oracle vs fp64): loss {bars['loss']:.2e} eig {bars['eig']:.2e} grad {bars['grad']:.2e}")
    return ref, bars


# ---------------------------------------------------------------- train()
def train_data(case):
    mode, data, k, model = case
    n = TRAIN["n_frames"] + (LAG if mode == "tr" else 0)
    return frames(data, n, TRAIN_SEED)


def train_loop(case, dtype):
    """The reference loop of train() in ``dtype``: dict(rows [epochs][train steps + test steps, 3 + k], eigs of the train steps,
    params {name: final tensor}, cvec of the last train step, xi: the CVs of the first 50 frames in cvec order)."""
    from oracle import nnref
    from oracle.train import split_indices
    mode, data, k, model = case
    lag = LAG if mode == "tr" else 0
    traj, w, ref = train_data(case)
    trunk, head, sd0 = init(data, k, model, TRAIN_SEED)
    torch.set_default_dtype(dtype)
    try:
        ol = oracle_layer(data, ref)
        X, wt = torch.tensor(traj, dtype=dtype), torch.tensor(w, dtype=dtype)
        sd = tie({n: p.to(dtype).clone().requires_grad_(True) for n, p in sd0.items()}, k, len(trunk) - 1)
        leaves = [sd[n] for n in param_names(case)]
        opt = torch.optim.Adam(leaves, lr=TRAIN["learning_rate"])
        np.random.seed(TRAIN["seed"])
        split_indices(len(traj) - lag, TRAIN["test_ratio"])
        idx_train, idx_test = split_indices(len(traj) - lag, TRAIN["test_ratio"])

        def batches(idx):
            bs = min(TRAIN["batch_size"], len(idx))
            return [] if bs == 0 else [torch.as_tensor(idx[s:s + bs], dtype=torch.long) for s in range(0, len(idx) - bs + 1, bs)]

        rows, cvec = [], None
        for _ in range(TRAIN["num_epochs"]):
            ep = []
            for train, idx in [(True, b) for b in batches(idx_train)] + [(False, b) for b in batches(idx_test)]:
                if train:
                    opt.zero_grad(set_to_none=True)
                lo, eo, no, po, co = _loss(sd, case, ol, X[idx], wt[idx], X[idx + lag], wt[idx + lag], dtype)
                if train:
                    cvec = [int(c) for c in co]
                    lo.backward()
                    opt.step()
                ep.append([float(lo.detach()), float(no.detach()), float(po.detach())] + [float(e) for e in eo])
            rows.append(np.asarray(ep))
        with torch.no_grad():
            xi = nnref.eigenfunctions_forward(nnref.reorder_eigenfunctions({n: p.detach() for n, p in sd.items()}, cvec), k, ol(X[:50]))
        params = {n: sd[n].detach().double().numpy() for n in param_names(case)}
    finally:
        torch.set_default_dtype(torch.float32)
    return dict(rows=np.stack(rows), params=params, cvec=cvec, xi=xi.double().numpy())


def centred(xi):
    """CVs up to their additive constants: the loss does not see an eigenfunction's output bias, whose gradient is roundoff."""
    return xi - xi.mean(axis=0, keepdims=True)


def train_errors(got, want, case):
    """(loss rows relative, final parameters / the largest, centred CVs / the largest) distances from the fp64 loop; the output biases
    are left out (exact gradient 0: Adam random-walks on roundoff in every precision)."""
    skip = output_biases(case)
    rows = float(np.max(np.abs(got["rows"] - want["rows"]) / np.abs(want["rows"])))
    pmax = max(float(np.abs(p).max()) for p in want["params"].values())
    par = max(float(np.abs(got["params"][n] - p).max()) for n, p in want["params"].items() if n not in skip) / pmax
    xi = float(np.abs(centred(got["xi"]) - centred(want["xi"])).max() / np.abs(centred(want["xi"])).max())
    return rows, par, xi


@functools.lru_cache(maxsize=None)
def train_reference():
    """({case: fp64 loop}, {case: bars}) - computed once per process, never modified."""
    ref, bars = {}, {}
    for case in TRAIN_CASES:
        ref[case] = want = train_loop(case, torch.float64)
        e = train_errors(train_loop(case, torch.float32), want, case)
        bars[case] = dict(zip(("rows", "params", "xi"), (8.0 * x for x in e)))
        print(f"[shared-task] train bars {case_id(case)}: " + " ".join(f"{n} {v:.2e}" for n, v in bars[case].items()))
    return ref, bars
