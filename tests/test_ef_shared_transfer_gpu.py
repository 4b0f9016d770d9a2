"""GPU (-m gpu): the transfer-mode shared-trunk entries of csrc/ef_general.hip (cvf_ef_general_shared_transfer_*, DESIGN.md section
4.12) through the C ABI - k scalar nets whose first n_shared Linear layers are one set of parameters, time-lagged loss.

The step is the one EigenFunctionTask runs on a SharedEigenFunctions model with lag_tau > 0: features -> 2T tiles (the frames, then
their lagged partners; cvf_align_feature_fwd on the identity layer), cvf_ef_general_shared_transfer_fwd, cvf_ef_stats (the batch
sums, the loss tail and its coefficients), cvf_ef_general_shared_transfer_backward, cvf_slab_reduce.

Cases, inputs, reference (oracle.losses.ef_loss in fp64, the shared layers the same leaf tensors for every net) and the bars (8 x the
fp32 CPU oracle's own distance from fp64, per quantity, computed where the test runs): tests/ef_shared_transfer_cases.py.  Every case
prints its achieved errors and the bars before it asserts.

Batches: 70 frames (two ragged tiles, four with the lagged ones) and tests/ef_general_cases.py::HALF_B = 64 * 128 + 37 frames (129
tiles, 258 step tiles on 256 slab rows: rows 0 and 1 add a lagged tile to a base tile).
"""
import numpy as np
import pytest
import torch

from tests import ef_shared_transfer_cases as S

pytestmark = pytest.mark.gpu
IDS = [c[0] for c in S.CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reference():
    return S.reference()


class Step:
    """One transfer-mode step through the C ABI.  ``ns`` = None: the plain entries (cvf_ef_general_fwd / _backward); else the
    shared transfer entries with that n_shared.  ``layout_ns``: n_shared of the flat layout ``theta`` is in (default: ns)."""

    def __init__(self, dev, dims, k, ns, act, theta, X, w, layout_ns=None):
        from colvarsfinder import _hip, core
        from colvarsfinder.pp import identity_desc
        lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
        lay = ns if layout_ns is None else layout_ns
        L = len(dims) - 1
        self.flat = fl = core._SharedTrunkFlat(dims, [S.ACTS[act][0]] * (L - 1) + [0], k, lay or 0, dev)
        assert fl.n == theta.numel()
        fl.theta.copy_(theta)
        B, D = X.shape[0] - S.LAG, X.shape[1]
        T = _hip.ntiles(B)
        nt = 2 * T
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        pp = identity_desc(D)
        rows, rows_lag = X[:B].to(dev).contiguous(), X[S.LAG:S.LAG + B].to(dev).contiguous()
        wd, wl = w[:B].to(dev).contiguous(), w[S.LAG:S.LAG + B].to(dev).contiguous()
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, S.LAG, 1, S.ALPHA, 1.0, S.DT
        for i, v in enumerate(S.eig_w(k)):
            cfg.eig_w[i] = v
        if ns is None:
            n_saved, n_rows = lib.cvf_ef_general_saved_floats(fl.desc, nt, S.LAG), lib.cvf_ef_general_slab_rows(fl.desc, nt)
        else:
            n_saved = lib.cvf_ef_general_shared_transfer_saved_floats(fl.desc, nt, ns)
            n_rows = lib.cvf_ef_general_shared_transfer_slab_rows(fl.desc, nt, ns)
        assert n_saved > 0 and n_rows >= 2, (n_saved, n_rows, lib.cvf_last_error())
        self.n_saved, self.n_rows, self.nt = n_saved, n_rows, nt
        feat = torch.empty(nt * D * 64, **f32)
        self.y = torch.full((nt * k * 64,), float("nan"), **f32)
        saved = torch.empty(n_saved, **f32)
        scratch = torch.zeros(lib.cvf_ef_stats_scratch_doubles(k, S.LAG), **f64)
        stats = torch.zeros(lib.cvf_ef_nstats(k, S.LAG), **f64)
        self.loss_vec, coef = torch.zeros(3 + 2 * k, **f64), torch.zeros(4 * k + k * k, **f64)
        self.slab = torch.full((n_rows * fl.n,), float("nan"), **f32)
        self.grad = torch.zeros(fl.n, **f32)
        _hip.check(lib.cvf_align_feature_fwd(pp, P(rows), B, P(feat), None, None, None, s), "cvf_align_feature_fwd")
        _hip.check(lib.cvf_align_feature_fwd(pp, P(rows_lag), B, P(feat[T * D * 64:]), None, None, None, s), "cvf_align_feature_fwd")
        if ns is None:
            _hip.check(lib.cvf_ef_general_fwd(fl.desc, P(fl.theta), P(feat), nt, P(self.y), None, P(saved), s), "fwd")
        else:
            _hip.check(lib.cvf_ef_general_shared_transfer_fwd(fl.desc, ns, P(fl.theta), P(feat), nt, P(self.y), P(saved), s), "shared fwd")
        _hip.check(lib.cvf_ef_stats(cfg, B, P(wd), P(self.y), None, P(wl), P(self.y[T * k * 64:]), P(scratch), P(stats), P(self.loss_vec),
                                    P(coef), s), "cvf_ef_stats")
        if ns is None:
            _hip.check(lib.cvf_ef_general_backward(cfg, fl.desc, P(fl.theta), B, P(wd), P(wl), P(feat), P(self.y), None, P(coef),
                                                   P(self.slab), None, P(saved), s), "backward")
        else:
            _hip.check(lib.cvf_ef_general_shared_transfer_backward(cfg, fl.desc, ns, P(fl.theta), B, P(wd), P(wl), P(feat), P(self.y),
                                                                   P(coef), P(self.slab), None, P(saved), s), "shared backward")
        _hip.check(lib.cvf_slab_reduce(P(self.slab), n_rows, fl.n, P(self.grad), None, s), "cvf_slab_reduce")
        torch.cuda.synchronize()

    def result(self, k):
        lv = self.loss_vec.cpu().numpy()
        return lv[:3], lv[3:3 + k], [int(c) for c in lv[3 + k:3 + 2 * k]], self.grad.double().cpu().numpy()


def _shared_step(dev, case, B):
    cid, dims, k, ns, act = case
    sd, X, w = S.inputs(cid, B)
    return Step(dev, dims, k, ns, act, S.flat(sd, dims, k, ns), X, w)


def _copies_step(dev, case, B, entries_ns):
    """The same nets as K explicit copies of the trunk (every net its own parameters), on the plain entries (None) or on the
    shared transfer entries with n_shared = 0."""
    cid, dims, k, ns0, act = case
    sd, X, w = S.inputs(cid, B)
    return Step(dev, dims, k, entries_ns, act, S.flat(S.tied(sd, k, ns0), dims, k, 0), X, w, layout_ns=0)


@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_shared_transfer_step_vs_fp64_oracle(dev, reference, case, B):
    ref, bars = reference
    cid, dims, k, ns, act = case
    st = _shared_step(dev, case, B)
    got, want = st.result(k), ref[cid, B]
    e_loss, e_eig, e_grad = S.errors(got, want)
    print(f"[shared-tr] {cid} B={B}: loss {e_loss:.2e} (bar {bars['loss']:.2e}) eig {e_eig:.2e} (bar {bars['eig']:.2e}) "
          f"grad {e_grad:.2e} (bar {bars['grad']:.2e}) rows {st.n_rows} saved {st.n_saved}")
    assert not torch.isnan(st.y).any() and not torch.isnan(st.slab).any()
    assert got[2] == want[2]
    assert e_loss <= bars["loss"] and e_eig <= bars["eig"] and e_grad <= bars["grad"]


@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("case", S.CASES[:4], ids=IDS[:4])
def test_shared_equals_copies_and_new_entries_equal_plain(dev, reference, case, B):
    """y of the shared run is that of the plain transfer entries on K explicit copies of the trunk, bit for bit, and so are the
    heads' blocks of the gradient (the same slab row count in both runs); the trunk's gradient is the copies' summed over the nets,
    within the gradient bar; n_shared = 0 through the new entries equals the plain entries in every output, bit for bit."""
    _, bars = reference
    cid, dims, k, ns, act = case
    sh, old, new0 = _shared_step(dev, case, B), _copies_step(dev, case, B, None), _copies_step(dev, case, B, 0)
    assert not torch.isnan(sh.y).any() and not torch.isnan(sh.slab).any()
    assert torch.equal(sh.y, old.y)
    assert sh.n_saved < old.n_saved and sh.n_rows == old.n_rows == new0.n_rows
    for name in ("y", "loss_vec", "slab", "grad"):
        assert torch.equal(getattr(new0, name), getattr(old, name)), name
    L = len(dims) - 1
    size = [dims[l + 1] * (dims[l] + 1) for l in range(L)]
    per, n_sh = sum(size), sum(size[:ns])
    n_head = per - n_sh
    for i in range(k):   # head i: behind the trunk in the shared layout, behind net i's own trunk in the copies layout
        mine = sh.grad[n_sh + i * n_head:n_sh + (i + 1) * n_head]
        assert torch.equal(mine, old.grad[i * per + n_sh:(i + 1) * per]), f"head {i}"
    folded = S.sum_copies(old.grad.double().cpu().numpy(), dims, k, ns)
    got = sh.grad.double().cpu().numpy()
    err = float(np.abs(got - folded).max() / np.abs(folded).max())
    print(f"[shared-tr] {cid} B={B}: shared gradient vs summed copies {err:.2e} (bar {bars['grad']:.2e})")
    assert err <= bars["grad"]


@pytest.mark.parametrize("ns", [1, 2])
def test_one_net_with_shared_layers_equals_no_sharing(dev, ns):
    """k = 1: the boundary launch (ns = 1) and the summed top step (ns = 2 = NH) on one net give the plain chain's bits."""
    dims = [7, 65, 33, 1]
    sd, X, w = S.inputs("d2-k3", 70)
    theta = S.flat(sd, dims, 1, 0)
    a, b = Step(dev, dims, 1, ns, "tanh", theta, X, w), Step(dev, dims, 1, 0, "tanh", theta, X, w)
    plain = Step(dev, dims, 1, None, "tanh", theta, X, w)
    for name in ("y", "loss_vec", "slab", "grad"):
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(plain, name)), name


@pytest.mark.parametrize("cid", ["d3-k8", "top-d2-k3"])
def test_two_runs_give_the_same_bits(dev, cid):
    case = S.case_of(cid)
    a, b = _shared_step(dev, case, S.BATCHES[1]), _shared_step(dev, case, S.BATCHES[1])
    assert torch.equal(a.slab, b.slab) and torch.equal(a.grad, b.grad) and torch.equal(a.loss_vec, b.loss_vec) and torch.equal(a.y, b.y)


def test_refusals_name_the_reason_and_launch_nothing(dev):
    """A generator-mode cfg, a missing w_lag, n_shared out of range, unequal offsets in a shared layer, overlapping unshared blocks:
    0 / a negative code and a reason, and the 7.0-filled output buffers keep their fill."""
    from colvarsfinder import _hip, core
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    dims, k, ns = [7, 65, 33, 1], 3, 1

    def desc():
        return core._SharedTrunkFlat(dims, [1, 1, 0], k, ns, dev)

    T, B = 2, 70
    nt = 2 * T
    f32 = dict(device=dev, dtype=torch.float32)
    fl = desc()
    feat = torch.zeros(nt * dims[0] * 64, **f32)
    y = torch.full((nt * k * 64,), 7.0, **f32)
    saved = torch.full((lib.cvf_ef_general_shared_transfer_saved_floats(fl.desc, nt, ns),), 7.0, **f32)
    slab = torch.full((nt * fl.n,), 7.0, **f32)
    wd, coef = torch.ones(B, **f32), torch.zeros(4 * k + k * k, device=dev, dtype=torch.float64)
    tr, gen = _hip.EFCfg(), _hip.EFCfg()
    tr.k, tr.lag_idx, tr.beta, tr.dt = k, 2, 1.0, 1.0
    gen.k, gen.lag_idx, gen.beta, gen.dt = k, 0, 1.0, 1.0

    def says(why):
        assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()

    def bwd(cfg, d, n, w_lag):
        return lib.cvf_ef_general_shared_transfer_backward(cfg, d, n, P(fl.theta), B, P(wd), P(w_lag), P(feat), P(y), P(coef), P(slab),
                                                           None, P(saved), s)

    def refused(d, n, why):
        assert lib.cvf_ef_general_shared_transfer_supported(d, n) == 0
        says(why)
        assert lib.cvf_ef_general_shared_transfer_saved_floats(d, nt, n) == 0 and lib.cvf_ef_general_shared_transfer_slab_rows(d, nt, n) == 0
        assert lib.cvf_ef_general_shared_transfer_fwd(d, n, P(fl.theta), P(feat), nt, P(y), P(saved), s) < 0
        says(why)
        assert bwd(tr, d, n, wd) < 0
        says(why)

    d = desc().desc
    d.w_off[1][0] += 1
    refused(d, ns, "offsets differ")
    d = desc().desc
    d.w_off[2][1] = d.w_off[1][1]
    refused(d, ns, "overlap")
    for n in (-1, 3):
        refused(desc().desc, n, "n_shared")
    assert bwd(gen, fl.desc, ns, wd) < 0
    says("generator-mode cfg")
    assert bwd(tr, fl.desc, ns, None) < 0
    says("needs w_lag")
    assert lib.cvf_ef_general_shared_transfer_supported(fl.desc, ns) == 1
    torch.cuda.synchronize()
    for t in (y, saved, slab):
        assert bool((t == 7.0).all())
