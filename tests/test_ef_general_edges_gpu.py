"""GPU (-m gpu): the per-layer eigenfunction kernels of csrc/ef_general.hip (efg_layer_kernel, efg_wgrad_kernel, efg_coef_kernel,
efg_top_kernel on the 64 x 64 core of csrc/cvf_gemm64.hpp) at their block edges, every case of tests/ef_general_cases.py through
the C ABI against the fp64 oracle (oracle.losses.ef_loss on the identity preprocessing).

The tiled inputs are built in torch (ef_general_cases.feat_tiled), so no other kernel stands between the table and the kernels
under test.  Generator mode: cvf_ef_general[_shared]_fwd -> cvf_metric_apply_stats on the identity layer (q = a .* g, the batch
sums, the loss tail and its coefficients) -> cvf_ef_general[_shared]_backward -> cvf_slab_reduce.  Transfer mode:
cvf_ef_general_fwd on 2T tiles without g_tiled -> cvf_ef_stats (the loss vector and coef) -> cvf_ef_general_backward with w_lag
-> cvf_slab_reduce.

Per case: y_tiled on the valid lanes and (generator mode) g_tiled against the fp64 forward and dy/dr, each relative to its
largest entry; the loss vector and the eigenvalues, relative; the reduced gradient as largest entry error over the largest
entry; the order of the eigenvalues.  y, g and the slab start as NaN and must be finite where the step owns them; saved, slab,
y and g each end in a zone of sentinels behind the size the library asked for, which must be untouched; the step counter goes up
by exactly one.  The bars are ef_general_cases.BARS (8 x the fp32 CPU oracle's own distance from the fp64 oracle, per group and
quantity); every case prints its achieved errors before it asserts, and with CVF_GENERAL_EDGE_ERRORS=<path> the module writes
them as JSON.
"""
import json
import os

import pytest
import torch

from tests import ef_general_cases as G

pytestmark = pytest.mark.gpu

GUARD = 1 << 14          # floats of sentinels behind every output buffer
SENTINEL = -1234.5
ERRORS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("CVF_GENERAL_EDGE_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(ERRORS, f, indent=1)


def _guarded(n, dev, fill=float("nan")):
    t = torch.full((n + GUARD,), SENTINEL, device=dev, dtype=torch.float32)
    t[:n] = fill
    return t


def _pad_lanes(t, tiles, lanes_from, value):
    """Write `value` into lanes `lanes_from`.. of the given tiles of a tiled tensor [tiles][...][64] (a view of it)."""
    for tile in tiles:
        t[tile, ..., lanes_from:] = value


class Step:
    """One step of a case through the C ABI (the plain entries for n_shared None, else the shared ones), built as
    test_ef_general_shared_gpu.Step builds its description and config.  `garbage`: finite garbage in the padded lanes of feat_tiled
    and q_tiled; `coef`: the loss coefficients of another run instead of this run's."""

    def __init__(self, dev, case, garbage=False, coef=None):
        from colvarsfinder import _hip, core
        from colvarsfinder.pp import identity_desc
        lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
        inp, k, ns, gen = G.inputs(case), case.k, case.ns, case.mode == "gen"
        D, B = case.dims[0], case.B
        T, nt = G.n_tiles(B), G.step_tiles(case)
        self.case, self.dev = case, dev
        self.flat = fl = core._SharedTrunkFlat(list(case.dims), G.act_codes(case), k, ns or 0, dev)
        theta = G.flat(inp.sd, case.dims, k, ns)
        assert fl.n == theta.numel() == G.n_params(case.dims, k, ns)
        fl.theta.copy_(theta)
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, 0 if gen else G.LAG, 1, G.ALPHA, G.BETA, 1.0 if gen else G.DT
        for i, v in enumerate(G.eig_w(k)):
            cfg.eig_w[i] = v
        if ns is None:
            n_saved, n_rows = lib.cvf_ef_general_saved_floats(fl.desc, nt, cfg.lag_idx), lib.cvf_ef_general_slab_rows(fl.desc, nt)
        else:
            n_saved, n_rows = lib.cvf_ef_general_shared_saved_floats(fl.desc, nt, ns), lib.cvf_ef_general_shared_slab_rows(fl.desc, nt, ns)
        assert n_saved == G.efg_layout(case.dims, k, nt, gen, ns).total and n_rows == G.g64_rows(fl.n, nt), lib.cvf_last_error()
        self.n_saved, self.n_rows, self.n_y, self.n_g, self.n_slab = n_saved, n_rows, nt * k * 64, T * k * D * 64, n_rows * fl.n
        pad = B - (T - 1) * 64       # first padded lane of a pass's last tile (64: none)
        feat = G.feat_tiled(case, inp).to(dev)
        if garbage:
            _pad_lanes(feat.view(nt, D, 64), [T - 1] if gen else [T - 1, 2 * T - 1], pad, -3.25)
        wd = inp.w.to(dev).contiguous()
        self.y, self.saved, self.slab = _guarded(self.n_y, dev), _guarded(n_saved, dev), _guarded(self.n_slab, dev)
        self.g = _guarded(self.n_g, dev) if gen else None
        self.loss_vec, self.coef = torch.zeros(3 + 2 * k, **f64), torch.zeros(4 * k + k * k, **f64)
        stats = torch.zeros(lib.cvf_ef_nstats(k, cfg.lag_idx), **f64)
        self.grad = torch.zeros(fl.n, **f32)
        self.step = torch.full((1,), 5, device=dev, dtype=torch.int32)
        if gen:
            pp, ad = identity_desc(D), inp.a.to(dev).contiguous()
            rows = inp.X.to(dev).contiguous()
            q, e = torch.zeros(self.n_g, **f32), torch.zeros(T * k * 64, **f32)
            scratch = torch.zeros(lib.cvf_metric_stats_scratch_doubles(B, k), **f64)
            if ns is None:
                _hip.check(lib.cvf_ef_general_fwd(fl.desc, P(fl.theta), P(feat), T, P(self.y), P(self.g), P(self.saved), s), "fwd")
            else:
                _hip.check(lib.cvf_ef_general_shared_fwd(fl.desc, ns, P(fl.theta), P(feat), T, P(self.y), P(self.g), P(self.saved), s),
                           "shared fwd")
            _hip.check(lib.cvf_metric_apply_stats(pp, P(rows), B, None, P(ad), k, P(self.g), P(q), P(e), None, None, cfg, P(wd),
                                                  P(self.y), P(scratch), P(stats), P(self.loss_vec), P(self.coef), s),
                       "cvf_metric_apply_stats")
            if garbage:
                _pad_lanes(q.view(T, k, D, 64), [T - 1], pad, 5.5)
            cf = self.coef if coef is None else coef
            if ns is None:
                _hip.check(lib.cvf_ef_general_backward(cfg, fl.desc, P(fl.theta), B, P(wd), None, P(feat), P(self.y), P(q), P(cf),
                                                       P(self.slab), P(self.step), P(self.saved), s), "backward")
            else:
                _hip.check(lib.cvf_ef_general_shared_backward(cfg, fl.desc, ns, P(fl.theta), B, P(wd), P(feat), P(self.y), P(q), P(cf),
                                                              P(self.slab), P(self.step), P(self.saved), s), "shared backward")
        else:
            wl = inp.w_lag.to(dev).contiguous()
            scratch = torch.zeros(lib.cvf_ef_stats_scratch_doubles(k, cfg.lag_idx), **f64)
            _hip.check(lib.cvf_ef_general_fwd(fl.desc, P(fl.theta), P(feat), nt, P(self.y), None, P(self.saved), s), "fwd")
            y_lag = self.y[T * k * 64:]
            _hip.check(lib.cvf_ef_stats(cfg, B, P(wd), P(self.y), None, P(wl), P(y_lag), P(scratch), P(stats), P(self.loss_vec),
                                        P(self.coef), s), "cvf_ef_stats")
            cf = self.coef if coef is None else coef
            _hip.check(lib.cvf_ef_general_backward(cfg, fl.desc, P(fl.theta), B, P(wd), P(wl), P(feat), P(self.y), None, P(cf),
                                                   P(self.slab), P(self.step), P(self.saved), s), "backward")
        _hip.check(lib.cvf_slab_reduce(P(self.slab), n_rows, fl.n, P(self.grad), None, s), "cvf_slab_reduce")
        torch.cuda.synchronize()

    def result(self):
        """The step's outputs in the shape of ef_general_cases.oracle's."""
        c, k = self.case, self.case.k
        lv = self.loss_vec.cpu().numpy()
        y = G.untile(self.y[:self.n_y].cpu(), k)[G.valid_rows(c)].double().numpy()
        g = None if self.g is None else G.untile(self.g[:self.n_g].cpu(), k, c.dims[0])[:c.B].double().numpy()
        return dict(y=y, g=g, lv=lv[:3], eig=lv[3:3 + k], cvec=[int(v) for v in lv[3 + k:3 + 2 * k]], grad=self.grad.double().cpu().numpy())

    def problems(self):
        """What the step left where it must not, or did not write where it must: a list of findings (empty: none)."""
        out = []
        for name, t, n in (("saved", self.saved, self.n_saved), ("slab", self.slab, self.n_slab), ("y", self.y, self.n_y),
                           ("g", self.g, self.n_g)):
            if t is not None and not bool((t[n:] == SENTINEL).all()):
                out.append(f"sentinels behind {name} overwritten")
        if not bool(torch.isfinite(self.slab[:self.n_slab]).all()):
            out.append("slab entries not finite (unwritten or NaN)")
        r = self.result()
        if not bool(torch.isfinite(torch.as_tensor(r["y"])).all()):
            out.append("valid lanes of y not finite")
        if r["g"] is not None and not bool(torch.isfinite(torch.as_tensor(r["g"])).all()):
            out.append("valid lanes of g not finite")
        if int(self.step.item()) != 6:
            out.append(f"step_count went from 5 to {int(self.step.item())}")
        return out


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_case_vs_fp64_oracle(dev, case):
    want, bars = G.reference(case), G.BARS[G.group(case)]
    st = Step(dev, case)
    got = st.result()
    e = ERRORS[case.id] = G.errors(got, want)
    print(f"[edges] {case.id} {list(case.dims)} k={case.k} {case.act} B={case.B} rows {st.n_rows} tiles {G.step_tiles(case)}: "
          + " ".join(f"{q} {e[q]:.2e} (bar {bars[q]:.2e})" for q in G.QUANTITIES if q in e))
    assert st.problems() == []
    assert got["cvec"] == want["cvec"]
    assert set(e) == set(bars)
    for q, v in e.items():
        assert v <= bars[q], f"{case.id} {q}: {v:.2e} > bar {bars[q]:.2e}"


@pytest.mark.parametrize("mode", ["gen", "tr"])
def test_two_runs_give_the_same_bits(dev, mode):
    a, b = Step(dev, G.RAGGED[mode]), Step(dev, G.RAGGED[mode])
    for name in ("y", "g", "saved", "slab", "grad", "loss_vec", "coef"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64),
                                                        y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int64)), name


@pytest.mark.parametrize("mode", ["gen", "tr"])
def test_padded_lanes_do_not_reach_the_gradient(dev, mode):
    """Finite garbage in the padded lanes of feat_tiled and q_tiled, the loss coefficients taken from the clean run: the slab and
    the gradient keep their bits, and so do the valid lanes of y and g."""
    case = G.RAGGED[mode]
    clean = Step(dev, case)
    dirty = Step(dev, case, garbage=True, coef=clean.coef)
    assert clean.problems() == [] and dirty.problems() == []
    assert torch.equal(dirty.slab[:dirty.n_slab].view(torch.int32), clean.slab[:clean.n_slab].view(torch.int32))
    assert torch.equal(dirty.grad.view(torch.int32), clean.grad.view(torch.int32))
    a, b = clean.result(), dirty.result()
    assert (a["y"] == b["y"]).all() and (mode == "tr" or (a["g"] == b["g"]).all())
    # ... and the garbage did reach the padded lanes of y: the check is not vacuous
    assert not torch.equal(dirty.y[:dirty.n_y], clean.y[:clean.n_y])
