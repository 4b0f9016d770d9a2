"""GPU (-m gpu): the shared-trunk entries of csrc/ef_general.hip (cvf_ef_general_shared_*) through the
C ABI - k scalar nets whose first n_shared Linear layers are one set of parameters, generator mode.

The step is the one RegAutoEncoderTask's gradient-norm penalty runs: features -> tiles (cvf_align_feature_fwd on the identity
layer), cvf_ef_general_shared_fwd (y, g = dy/dr), cvf_metric_apply_stats (q = A g, the batch sums, the loss tail and its
coefficients), cvf_ef_general_shared_backward, cvf_slab_reduce.

Reference: oracle.losses.ef_loss in fp64 with the shared layers passed as the SAME leaf tensors for every net, so autograd sums
their gradient.  Bars, one per quantity, computed where the test runs (as tests/test_cv_nets_gpu.py does): 8 x the worst distance
of the same oracle evaluated in fp32 on the CPU from its fp64 evaluation, over all cases and both batch sizes - the loss vector
and the eigenvalues relative, the gradient relative to its largest entry.  Every case prints its achieved errors and the bars
before it asserts.

Batches: 70 frames (two tiles, a ragged tail) and 16 453 frames (258 tiles on 256 slab rows: rows 0 and 1 sum two tiles each).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = {"tanh": (1, torch.tanh), "relu": (3, torch.relu), "softplus": (6, F.softplus)}   # (code of include/cvf.h, oracle function)
# id, dims, k, n_shared, activation
CASES = [("d2-k3", [7, 65, 33, 1], 3, 1, "tanh"), ("all-shared", [9, 130, 1], 2, 1, "tanh"), ("d3-k8", [5, 5, 70, 6, 1], 8, 2, "tanh"),
         ("softplus", [7, 65, 33, 1], 3, 1, "softplus"), ("relu", [9, 130, 1], 2, 1, "relu")]
BATCHES = [70, 64 * 257 + 5]
ALPHA, BETA = 12.0, 1.2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _eig_w(k):
    return [1.0 - 0.1 * i for i in range(k)]


def _inputs(case, B):
    """Parameters (net 0's first n_shared layers stand for every net's), features, weights and metric of a case: CPU, fp32."""
    from oracle import nnref
    cid, dims, k, ns, act = case
    g = torch.Generator().manual_seed(1000 + 7 * CASES.index(case) + B % 97)
    sd = nnref.init_eigenfunctions(dims, k, g)
    X = torch.randn(B, dims[0], generator=g)
    w = torch.rand(B, generator=g) + 0.5
    a = torch.rand(dims[0], generator=g) + 0.5
    return sd, X, w, a


def _flat(sd, dims, k, ns):
    """Flat vector in the layout of core._SharedTrunkFlat: the shared layers once (net 0's), then net by net the rest."""
    L = len(dims) - 1
    out = [sd[f"eigen_funcs.0.{l + 1}.{n}"].reshape(-1) for l in range(ns) for n in ("weight", "bias")]
    for i in range(k):
        out += [sd[f"eigen_funcs.{i}.{l + 1}.{n}"].reshape(-1) for l in range(ns, L) for n in ("weight", "bias")]
    return torch.cat(out)


def _oracle(case, B, dtype):
    """(loss vector [loss, npl, pen], eigenvalues, cvec, flat gradient) of oracle.losses.ef_loss in ``dtype``."""
    from oracle import losses
    cid, dims, k, ns, act = case
    sd0, X, w, a = _inputs(case, B)
    torch.set_default_dtype(dtype)
    try:
        sd = {n: p.to(dtype).requires_grad_(True) for n, p in sd0.items()}
        for i in range(1, k):      # the same leaves: autograd sums the nets' gradients of a shared layer
            for l in range(ns):
                for n in ("weight", "bias"):
                    sd[f"eigen_funcs.{i}.{l + 1}.{n}"] = sd[f"eigen_funcs.0.{l + 1}.{n}"]
        Xo = X.to(dtype).requires_grad_(True)
        lo, eo, no, po, co = losses.ef_loss(sd, k, lambda x: x, Xo, w.to(dtype), alpha=ALPHA, eig_w=_eig_w(k), diag_coeff=a.to(dtype),
                                            beta=BETA, activation=ACTS[act][1])
        lo.backward()
        grad = _flat({n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in sd.items()}, dims, k, ns)
    finally:
        torch.set_default_dtype(torch.float32)
    return (np.asarray([float(lo), float(no), float(po)]), eo.double().numpy(), [int(c) for c in co], grad.double().numpy())


def _errors(got, want):
    """(loss vector, eigenvalues, gradient / its largest entry) distances of a result from the fp64 one."""
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))   # noqa: E731
    return rel(got[0], want[0]), rel(got[1], want[1]), float(np.abs(got[3] - want[3]).max() / np.abs(want[3]).max())


@pytest.fixture(scope="module")
def reference():
    """fp64 oracle of every (case, batch) - computed once, shared by the tests, never modified - and the three bars."""
    ref, worst = {}, [0.0, 0.0, 0.0]
    for case in CASES:
        for B in BATCHES:
            ref[case[0], B] = want = _oracle(case, B, torch.float64)
            worst = [max(a, b) for a, b in zip(worst, _errors(_oracle(case, B, torch.float32), want))]
    bars = dict(zip(("loss", "eig", "grad"), (8.0 * e for e in worst)))
    print(f"[shared] bars (8 x fp32 CPU oracle vs fp64): loss {bars['loss']:.2e} eig {bars['eig']:.2e} grad {bars['grad']:.2e}")
    return ref, bars


class Step:
    """One step through the C ABI.  ``ns`` = None: the plain entries (cvf_ef_general_fwd / _backward); else the shared ones."""

    def __init__(self, dev, dims, k, ns, act, theta, X, w, a, layout_ns=None):
        from colvarsfinder import _hip, core
        from colvarsfinder.pp import identity_desc
        lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
        lay = ns if layout_ns is None else layout_ns
        L = len(dims) - 1
        self.flat = fl = core._SharedTrunkFlat(dims, [ACTS[act][0]] * (L - 1) + [0], k, lay or 0, dev)
        assert fl.n == theta.numel()
        fl.theta.copy_(theta)
        B, D = X.shape
        T = _hip.ntiles(B)
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        pp = identity_desc(D)
        rows, wd, ad = X.to(dev).contiguous(), w.to(dev).contiguous(), a.to(dev).contiguous()
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, 0, 1, ALPHA, BETA, 1.0
        for i, v in enumerate(_eig_w(k)):
            cfg.eig_w[i] = v
        if ns is None:
            n_saved, n_rows = lib.cvf_ef_general_saved_floats(fl.desc, T, 0), lib.cvf_ef_general_slab_rows(fl.desc, T)
        else:
            n_saved, n_rows = lib.cvf_ef_general_shared_saved_floats(fl.desc, T, ns), lib.cvf_ef_general_shared_slab_rows(fl.desc, T, ns)
        assert n_saved > 0 and n_rows >= 2, (n_saved, n_rows, lib.cvf_last_error())
        self.n_saved, self.n_rows = n_saved, n_rows
        feat = torch.empty(T * D * 64, **f32)
        self.y, self.g = torch.full((T * k * 64,), float("nan"), **f32), torch.full((T * k * D * 64,), float("nan"), **f32)
        q, e = torch.empty(T * k * D * 64, **f32), torch.empty(T * k * 64, **f32)
        saved = torch.empty(n_saved, **f32)
        scratch = torch.zeros(lib.cvf_metric_stats_scratch_doubles(B, k), **f64)
        stats = torch.zeros(lib.cvf_ef_nstats(k, 0), **f64)
        self.loss_vec, coef = torch.zeros(3 + 2 * k, **f64), torch.zeros(4 * k + k * k, **f64)
        self.slab = torch.full((n_rows * fl.n,), float("nan"), **f32)
        self.grad = torch.zeros(fl.n, **f32)
        _hip.check(lib.cvf_align_feature_fwd(pp, P(rows), B, P(feat), None, None, None, s), "cvf_align_feature_fwd")
        if ns is None:
            _hip.check(lib.cvf_ef_general_fwd(fl.desc, P(fl.theta), P(feat), T, P(self.y), P(self.g), P(saved), s), "fwd")
        else:
            _hip.check(lib.cvf_ef_general_shared_fwd(fl.desc, ns, P(fl.theta), P(feat), T, P(self.y), P(self.g), P(saved), s), "shared fwd")
        _hip.check(lib.cvf_metric_apply_stats(pp, P(rows), B, None, P(ad), k, P(self.g), P(q), P(e), None, None, cfg, P(wd), P(self.y),
                                              P(scratch), P(stats), P(self.loss_vec), P(coef), s), "cvf_metric_apply_stats")
        if ns is None:
            _hip.check(lib.cvf_ef_general_backward(cfg, fl.desc, P(fl.theta), B, P(wd), None, P(feat), P(self.y), P(q), P(coef),
                                                   P(self.slab), None, P(saved), s), "backward")
        else:
            _hip.check(lib.cvf_ef_general_shared_backward(cfg, fl.desc, ns, P(fl.theta), B, P(wd), P(feat), P(self.y), P(q), P(coef),
                                                          P(self.slab), None, P(saved), s), "shared backward")
        _hip.check(lib.cvf_slab_reduce(P(self.slab), n_rows, fl.n, P(self.grad), None, s), "cvf_slab_reduce")
        torch.cuda.synchronize()

    def result(self, k):
        lv = self.loss_vec.cpu().numpy()
        return lv[:3], lv[3:3 + k], [int(c) for c in lv[3 + k:3 + 2 * k]], self.grad.double().cpu().numpy()


def _shared_step(dev, case, B, ns=None):
    cid, dims, k, ns0, act = case
    ns = ns0 if ns is None else ns
    sd, X, w, a = _inputs(case, B)
    return Step(dev, dims, k, ns, act, _flat(sd, dims, k, ns), X, w, a)


def _copies_step(dev, case, B, entries_ns):
    """The same nets as K explicit copies of the trunk (every net its own parameters), on the plain entries (None) or on the
    shared entries with n_shared = 0."""
    cid, dims, k, ns0, act = case
    sd, X, w, a = _inputs(case, B)
    for i in range(1, k):
        for l in range(ns0):
            for n in ("weight", "bias"):
                sd[f"eigen_funcs.{i}.{l + 1}.{n}"] = sd[f"eigen_funcs.0.{l + 1}.{n}"]
    return Step(dev, dims, k, entries_ns, act, _flat(sd, dims, k, 0), X, w, a, layout_ns=0)


def _sum_copies(grad, dims, k, ns):
    """Gradient of the copies layout folded into the shared layout: the nets' copies of the shared layers summed."""
    L = len(dims) - 1
    size = [dims[l + 1] * (dims[l] + 1) for l in range(L)]
    per, n_sh = sum(size), sum(size[:ns])
    g = grad.reshape(k, per)
    return np.concatenate([g[:, :n_sh].sum(0)] + [g[i, n_sh:] for i in range(k)])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shared_step_vs_fp64_oracle(dev, reference, case, B):
    ref, bars = reference
    cid, dims, k, ns, act = case
    st = _shared_step(dev, case, B)
    got, want = st.result(k), ref[cid, B]
    e_loss, e_eig, e_grad = _errors(got, want)
    print(f"[shared] {cid} B={B}: loss {e_loss:.2e} (bar {bars['loss']:.2e}) eig {e_eig:.2e} (bar {bars['eig']:.2e}) "
          f"grad {e_grad:.2e} (bar {bars['grad']:.2e}) rows {st.n_rows} saved {st.n_saved}")
    assert got[2] == want[2]
    assert e_loss <= bars["loss"] and e_eig <= bars["eig"] and e_grad <= bars["grad"]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_shared_equals_copies_and_new_entries_equal_old(dev, reference, case, B):
    """y and g of the shared run are those of the plain entries on K explicit copies of the trunk, bit for bit; n_shared = 0 through
    the new entries equals the plain entries in every output; the shared gradient is the sum of the copies' within the bar."""
    _, bars = reference
    cid, dims, k, ns, act = case
    sh, old, new0 = _shared_step(dev, case, B), _copies_step(dev, case, B, None), _copies_step(dev, case, B, 0)
    assert not torch.isnan(sh.y).any() and not torch.isnan(sh.g).any() and not torch.isnan(sh.slab).any()
    assert torch.equal(sh.y, old.y) and torch.equal(sh.g, old.g)
    assert sh.n_saved < old.n_saved
    for name in ("y", "g", "loss_vec", "slab", "grad"):
        assert torch.equal(getattr(new0, name), getattr(old, name)), name
    folded = _sum_copies(old.grad.double().cpu().numpy(), dims, k, ns)
    got = sh.grad.double().cpu().numpy()
    err = float(np.abs(got - folded).max() / np.abs(folded).max())
    print(f"[shared] {cid} B={B}: shared gradient vs summed copies {err:.2e} (bar {bars['grad']:.2e})")
    assert err <= bars["grad"]


def test_one_net_with_shared_layers_equals_no_sharing(dev):
    case = ("k1", [7, 65, 33, 1], 1, 2, "tanh")
    sd, X, w, a = _inputs(CASES[0], 70)
    theta = _flat(sd, case[1], 1, 0)
    s2, s0 = Step(dev, case[1], 1, 2, "tanh", theta, X, w, a), Step(dev, case[1], 1, 0, "tanh", theta, X, w, a)
    for name in ("y", "g", "loss_vec", "slab", "grad"):
        assert torch.equal(getattr(s2, name), getattr(s0, name)), name


def test_two_runs_give_the_same_bits(dev):
    a, b = _shared_step(dev, CASES[2], BATCHES[1]), _shared_step(dev, CASES[2], BATCHES[1])
    assert torch.equal(a.slab, b.slab) and torch.equal(a.grad, b.grad) and torch.equal(a.loss_vec, b.loss_vec)


def test_refusals_name_the_reason_and_launch_nothing(dev):
    """Unequal offsets in a shared layer, overlapping unshared blocks, n_shared out of range, a transfer-mode cfg (the predicate
    takes no cfg: the backward entry refuses it, and the forward entry a call without g_tiled): 0 / a negative code and a
    reason, and the output buffers keep their fill."""
    from colvarsfinder import _hip, core
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    dims, k, ns = [7, 65, 33, 1], 3, 1

    def desc():
        return core._SharedTrunkFlat(dims, [1, 1, 0], k, ns, dev)

    T, B = 2, 70
    f32 = dict(device=dev, dtype=torch.float32)
    fl = desc()
    feat = torch.zeros(T * dims[0] * 64, **f32)
    y, g = torch.full((T * k * 64,), 7.0, **f32), torch.full((T * k * dims[0] * 64,), 7.0, **f32)
    saved = torch.full((lib.cvf_ef_general_shared_saved_floats(fl.desc, T, ns),), 7.0, **f32)
    slab = torch.full((T * fl.n,), 7.0, **f32)
    wd, coef = torch.ones(B, **f32), torch.zeros(4 * k + k * k, device=dev, dtype=torch.float64)
    cfg = _hip.EFCfg()
    cfg.k, cfg.lag_idx, cfg.beta, cfg.dt = k, 0, 1.0, 1.0

    def refused(d, n, why, c=cfg, gt=g):
        if c is cfg and gt is g:
            assert lib.cvf_ef_general_shared_supported(d, n) == 0
            assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()
            assert lib.cvf_ef_general_shared_saved_floats(d, T, n) == 0 and lib.cvf_ef_general_shared_slab_rows(d, T, n) == 0
        if c is cfg:
            assert lib.cvf_ef_general_shared_fwd(d, n, P(fl.theta), P(feat), T, P(y), P(gt), P(saved), s) < 0
            assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()
        if gt is g:
            assert lib.cvf_ef_general_shared_backward(c, d, n, P(fl.theta), B, P(wd), P(feat), P(y), P(g), P(coef), P(slab), None,
                                                      P(saved), s) < 0
            assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()

    d = desc().desc
    d.w_off[1][0] += 1
    refused(d, ns, "offsets differ")
    d = desc().desc
    d.w_off[2][1] = d.w_off[1][1]
    refused(d, ns, "overlap")
    for n in (-1, 3):
        refused(desc().desc, n, "n_shared")
    tr = _hip.EFCfg()
    tr.k, tr.lag_idx, tr.beta, tr.dt = k, 2, 1.0, 1.0
    refused(fl.desc, ns, "transfer-mode", c=tr)
    refused(fl.desc, ns, "transfer-mode", gt=None)
    assert lib.cvf_ef_general_shared_supported(fl.desc, ns) == 1
    torch.cuda.synchronize()
    for t in (y, g, saved, slab):
        assert bool((t == 7.0).all())
