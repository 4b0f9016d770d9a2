"""GPU (-m gpu): one cvf_ae_step per case of tests/ae_cases.py against the fp64 oracle (oracle.losses.ae_loss with autograd) -
every compiled ae16_kernel<RTD, RTH> and ae_mfma_kernel<TANH> instance, both LDS layouts of the latter, with and without the
gradient, with and without the `idx` gather, on batches from 1 frame to more than 2048 tiles.

The step is called through the C ABI with the arguments AutoEncoderTask._step passes, so that every buffer can sit between
guard bands inside a larger tensor and theta can start off a 16-byte line.  Each case asserts
  - the route: cvf_ae_step_route() - the function cvf_ae_step itself decides by - answers what ae_cases.route() predicts, LDS
    bytes included, so a shape that fell back to the other kernel cannot pass as coverage;
  - loss and every gradient entry against fp64, at the group's bar of ae_cases.BARS (8 x the fp32 CPU oracle's own distance from
    fp64; see there); loss-only cases: the loss, and that grad and step_count were left alone;
  - no reliance on stale memory: the scratch buffer starts as NaN; refilled with NaN and then used by another chain on a larger
    grid, it gives the same bits as the call on fresh scratch; two calls give the same bits;
  - containment: the guard bands around grad, out2 and scratch are intact;
  - `dup` cases: two copies of the batch give the same loss and gradient (bars of test_large_batch_paths_by_duplication);
  - `adam` cases: three fused Adam steps against three torch.optim.Adam steps of the fp64 oracle (parameter bar of
    test_ae_train_trace), step_count advancing by one per step;
  - the refused chain: the library's error names the LDS need, and the next launch works.

Worst errors against fp64 per group, measured on an MI355X (worst e32: the fp32 CPU oracle's, the source of the bar):

  group                 cases   loss: worst e32   bar      achieved    gradient: worst e32   bar      achieved
  ae16, B < 1000        31      8.5e-08           6.9e-07  2.2e-08     2.0e-07               1.7e-06  3.0e-07
  ae16, B >= 1000       13      3.9e-08           3.2e-07  2.4e-09     6.4e-08               5.2e-07  2.3e-07
  mfma_tanh, B < 1000   13      9.1e-08           7.3e-07  3.6e-08     2.1e-07               1.7e-06  2.0e-07
  mfma_tanh, B >= 1000  6       5.3e-09           4.3e-08  9.7e-10     5.3e-08               4.3e-07  1.4e-07
  mfma_any, B < 1000    11      5.6e-08           4.6e-07  1.2e-08     1.4e-07               1.1e-06  1.6e-07
  mfma_any, B >= 1000   6       2.0e-08           1.7e-07  1.6e-09     8.4e-08               6.8e-07  1.8e-07

Three fused Adam steps (6 cases): final parameters within 6.5e-08 of the fp64 oracle's (bar 2e-06).

RegAutoEncoderTask's launch modes (10 cases, first step; bars: ae_cases.REGAE_BARS), worst over the cases:

  term        loss     ae       npl      pen      eig      norm     orth     grad
  worst e32   2.4e-06  5.1e-08  1.4e-05  5.5e-09  2.1e-05  1.9e-08  4.6e-07  3.5e-05
  bar         2.0e-05  4.1e-07  1.2e-04  4.5e-08  1.7e-04  1.5e-07  3.8e-06  2.8e-04
  achieved    3.6e-07  1.5e-08  1.1e-06  2.3e-09  1.6e-06  7.7e-09  2.3e-07  4.7e-06

What the sweep sees of the input padding (one-line mutations of ae16_kernel, each run through this module once): the mask on
the padded input units is applied in two places, the prologue's load of a block's first tile and load_frame for its later tiles.
Without the first, the 30 ae16 cases whose d0 is not a multiple of 4 fail and the 14 others pass (the first layer's k loop stops
at ceil(d0 / 4) steps, so padded units of a d0 that is a multiple of 4 never meet a weight); without the second, only a case
with more than 2048 tiles and such a d0 can fail (ae16-edge-B-big, ae16-edge-B-big-idx-loss).

The whole module (91 cases, the fp64 and fp32 oracles of the 140 000-frame batches included) takes 8 s on an MI355X; run it under
`timeout -k 10 120`.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ae_cases as A
from tests import ae_inputs as I
from tests import sweep_errors

pytestmark = pytest.mark.gpu

DUP_TOL = dict(loss=2e-6, grad=1e-4, grad_abs=2e-6)   # test_gpu_parity.py::test_large_batch_paths_by_duplication
ADAM_TOL = 2e-6      # test_gpu_parity.py::test_ae_train_trace: final parameters, rtol = atol
ADAM_LR, ADAM_STEPS = 1e-3, 3
GUARD = 64           # elements on either side of a guarded buffer (keeps the 16-byte alignment of what lies between)
SENTINEL = -7.25e9
POLLUTER = A.Case("polluter", (3, 2), (2, 3), "tanh", 0, False, True, False, False, False, False)
COUNT0 = 1000        # where step_count starts: a loss-only call must leave exactly this
ERRORS = {}          # case id -> {quantity: error}; merged into $CVF_SWEEP_ERRORS when set


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    sweep_errors.write(ERRORS)


class Guarded:
    """`n` elements between two bands of sentinels inside one allocation."""

    def __init__(self, n, dtype, dev, fill):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


class Step:
    """The device buffers of one case and the call."""

    def __init__(self, case, inp, dev, copies=1):
        from colvarsfinder import _hip
        rows, idx, wb, sd0 = inp
        self.case, self.dev, self.lib, self.desc = case, dev, _hip.lib(), I.mlp_desc(case)
        flat = torch.cat([p.reshape(-1) for p in sd0.values()])
        self.n = flat.numel()
        assert self.n == self.desc.n_params == A.n_params(A.dims(case))
        store = torch.zeros(self.n + 8, device=dev)          # (fresh allocations are 256-byte aligned)
        assert store.data_ptr() % 16 == 0
        self.theta = store[1:1 + self.n] if case.misaligned else store[:self.n]
        self.theta.copy_(flat)
        self.rows = torch.as_tensor(rows).to(dev)
        self.idx = None if idx is None else torch.as_tensor(np.concatenate([idx] * copies)).to(dev)
        if idx is None and copies > 1:
            self.rows = torch.cat([self.rows] * copies)
        self.w = torch.as_tensor(np.concatenate([wb] * copies)).to(dev)
        self.B = case.B * copies
        self.inv_wsum = 1.0 / float(self.w.sum(dtype=torch.float64))
        need = self.lib.cvf_ae_scratch_floats(self.desc, self.B)
        assert need == A.scratch_floats(A.dims(case), self.B)
        self.pol_B = min(A.grid(self.B)[0] + 8, A.MAX_BLOCKS) * A.TILE - 3
        self.pol_desc = I.mlp_desc(POLLUTER)
        self.scratch = Guarded(max(need, self.lib.cvf_ae_scratch_floats(self.pol_desc, self.pol_B)), torch.float32, dev, float("nan"))
        self.grad = Guarded(self.n, torch.float32, dev, SENTINEL)
        self.out2 = Guarded(3, torch.float64, dev, SENTINEL)
        self.count = torch.full((1,), COUNT0, dtype=torch.int32, device=dev)

    def route(self):
        lds = C.c_int64(-1)
        return self.lib.cvf_ae_step_route(self.desc, C.c_void_p(self.theta.data_ptr()), int(self.case.grad), C.byref(lds)), lds.value

    def call(self, adam=None):
        """-> (out2 [3] float64, gradient float32 or None) as numpy, bit copies."""
        from colvarsfinder import _hip
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _hip.check(self.lib.cvf_ae_step(self.desc, p(self.theta), p(self.rows), p(self.idx), self.B, p(self.w), self.inv_wsum,
                                        p(self.scratch.view), p(self.out2.view), p(self.grad.view) if self.case.grad else None,
                                        p(self.count), adam, _hip.stream()), "cvf_ae_step")
        torch.cuda.synchronize()
        return self.out2.view.cpu().numpy().copy(), (self.grad.view.cpu().numpy().copy() if self.case.grad else None)

    def pollute(self):
        """Another chain on a larger grid (the same 2048 blocks where the case has them all), gradient asked for, on this scratch."""
        from colvarsfinder import _hip
        p = lambda t: C.c_void_p(t.data_ptr())
        theta = torch.linspace(-0.5, 0.5, self.pol_desc.n_params, device=self.dev)
        rows = torch.rand(self.pol_B, 3, device=self.dev)
        w = torch.ones(self.pol_B, device=self.dev)
        g, o = torch.zeros(self.pol_desc.n_params, device=self.dev), torch.zeros(3, dtype=torch.float64, device=self.dev)
        _hip.check(self.lib.cvf_ae_step(self.pol_desc, p(theta), p(rows), None, self.pol_B, p(w), 1.0 / self.pol_B,
                                        p(self.scratch.view), p(o), p(g), None, None, _hip.stream()), "cvf_ae_step (polluter)")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(g).all())

    def intact(self):
        return self.scratch.intact() and self.grad.intact() and self.out2.intact()

    def adam_args(self, m, v):
        from colvarsfinder import _hip
        a = _hip.AdamArgs()
        a.theta, a.m, a.v = self.theta.data_ptr(), m.data_ptr(), v.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = ADAM_LR, 0.9, 0.999, 1e-8   # torch.optim.Adam's defaults, as core.py:164 builds it
        a.step_count = self.count.data_ptr()
        return a


def _same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and (a[1] is None or a[1].tobytes() == b[1].tobytes())


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_ae_step_vs_fp64_oracle(dev, case, monkeypatch):
    from colvarsfinder import _hip
    if case.no_ae16:
        monkeypatch.setenv("CVF_NO_AE16", "1")
    else:
        monkeypatch.delenv("CVF_NO_AE16", raising=False)
    inp = I.inputs(case)
    st = Step(case, inp, dev)
    code, lds = st.route()
    assert (code, lds) == (A.route_code(case), A.lds_bytes(case)), (case.id, code, lds, A.route(case))

    if A.route(case) == "refused":
        with pytest.raises(RuntimeError, match=rf"needs {A.lds_bytes(case)} B of LDS"):
            st.call()
        torch.cuda.synchronize()
        assert st.intact() and bool(torch.isnan(st.scratch.view).all()) and bool((st.grad.view == SENTINEL).all())
        st.pollute()                                      # no sticky error: the next launch runs and is checked
        return

    fresh = st.call()
    assert st.intact(), "a guard band around grad, out2 or scratch was written"
    assert int(st.count) == COUNT0 + int(case.grad)       # advanced once per gradient, never by a loss-only call
    if not case.grad:
        assert bool((st.grad.view == SENTINEL).all())
    again = st.call()
    assert _same_bits(fresh, again), "two calls on the same inputs differ"
    st.scratch.view.fill_(float("nan"))                   # nothing of the case's own earlier calls is left: NaN, then the
    st.pollute()                                          # other chain's slab rows and partials
    stale = st.call()
    assert _same_bits(fresh, stale), "the step read scratch memory it had not written"
    assert st.intact() and int(st.count) == COUNT0 + 3 * int(case.grad)

    # ---- values
    ref = I.oracle(case, inp, torch.float64, ADAM_STEPS if case.adam else 0, ADAM_LR)
    e32 = I.e32(case, inp, ref)
    out2, grad = fresh
    assert np.isfinite(out2).all() and (grad is None or np.isfinite(grad).all())
    np.testing.assert_allclose(out2[1], float(np.asarray(inp[2], dtype=np.float64).sum()), rtol=1e-12)
    np.testing.assert_allclose(out2[2], out2[0] / out2[1], rtol=1e-14)
    gmax = float(np.abs(ref[1]).max())
    e_loss = abs(out2[2] - ref[0]) / abs(ref[0])
    e_grad = float(np.abs(grad - ref[1]).max()) / gmax if case.grad else None
    ERRORS[case.id] = dict(group="/".join(A.group(case)), e32_loss=e32[0], e32_grad=e32[1], loss=e_loss, grad=e_grad)
    print(f"{case.id}: loss {e_loss:.2e} (e32 {e32[0]:.2e}), gradient {e_grad if e_grad is None else format(e_grad, '.2e')} (e32 {e32[1]:.2e})")
    t_loss, t_grad = A.BARS[A.group(case)]
    np.testing.assert_allclose(out2[2], ref[0], rtol=t_loss)
    if case.grad:
        np.testing.assert_allclose(grad, ref[1], rtol=0, atol=t_grad * gmax)

    # ---- two copies of the batch: every sum doubles, the loss is a ratio of sums
    if case.dup:
        st2 = Step(case, inp, dev, copies=2)
        assert st2.route() == (code, lds)
        o2, g2 = st2.call()
        assert st2.intact() and int(st2.count) == COUNT0 + int(case.grad)
        ERRORS[case.id].update(dup_loss=abs(o2[2] - ref[0]) / abs(ref[0]))
        np.testing.assert_allclose(o2[2], ref[0], rtol=t_loss)
        np.testing.assert_allclose(o2[2], out2[2], rtol=DUP_TOL["loss"])
        if case.grad:
            ERRORS[case.id].update(dup_grad=float(np.abs(g2 - ref[1]).max()) / gmax)
            np.testing.assert_allclose(g2, ref[1], rtol=0, atol=t_grad * gmax)
            np.testing.assert_allclose(g2, grad, rtol=DUP_TOL["grad"], atol=DUP_TOL["grad_abs"] * np.abs(grad).max())
        if A.grid(case.B)[1] > 1:
            assert A.grid(2 * case.B)[1] > A.grid(case.B)[1]

    # ---- three fused Adam steps
    if case.adam:
        sa = Step(case, inp, dev)
        m, v = torch.zeros(sa.n, device=dev), torch.zeros(sa.n, device=dev)
        sa.count.zero_()                                  # Adam's t: the gradient launch makes it 1 for the first update
        for step in range(ADAM_STEPS):
            sa.call(sa.adam_args(m, v))
            assert int(sa.count) == step + 1
        assert sa.intact()
        got = sa.theta.cpu().numpy().astype(np.float64)
        ERRORS[case.id].update(adam=float(np.abs(got - ref[2]).max()))
        np.testing.assert_allclose(got, ref[2], rtol=ADAM_TOL, atol=ADAM_TOL)


# ---------------------------------------------------------------------------------------------------- RegAutoEncoderTask
class _PlainPair:
    """The library with the hand-off calls of a step replaced by the plain forward / backward pair (same arguments)."""
    _plain = {"cvf_regae_forward_keep": "cvf_regae_forward", "cvf_regae_backward_reuse": "cvf_regae_backward"}

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, self._plain.get(name, name))


@pytest.mark.parametrize("case", A.REGAE_CASES, ids=[c.id for c in A.REGAE_CASES])
def test_regae_first_step_vs_fp64_oracle(dev, case, monkeypatch):
    """The launch modes of ae_mfma_kernel that RegAutoEncoderTask adds: K heads, lagged targets and inputs, 2 T tiles."""
    from colvarsfinder import _hip, core, nn
    from tests.synth import Traj
    c, h = case, I.REGAE_HYPER
    inp = I.regae_inputs(c)
    traj, w, idx, eig_w, sd0 = inp
    e_dims, d_dims, r_dims, chain = A.regae_dims(c)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, c.K)
    model.load_state_dict(sd0)
    task = core.RegAutoEncoderTask(Traj(traj, w, h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w,
                                   learning_rate=1e-3, batch_size=64, num_epochs=1, alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"],
                                   lag_tau_ae=c.lag_ae * h["dt"], lag_tau_reg=c.lag_reg * h["dt"], device=dev, verbose=False,
                                   save_model_every_step=0)
    desc = task._flat.desc
    assert list(desc.dims[:desc.n_layers + 1]) == chain
    assert A.mfma_layout(chain, True)[0] == c.layout and A.mfma_layout(chain, True)[1] <= A.MFMA_LDS_MAX
    W = task._weights

    def step(copies=1):
        it = torch.as_tensor(np.concatenate([idx] * copies), device=dev)
        B = it.numel()
        ws = task._workspace(B)
        guarded = Guarded(ws["scratch"].numel(), torch.float32, dev, float("nan"))
        ws["scratch"] = guarded.view
        row = task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg,
                         with_grad=True).cpu().numpy()
        task.backward()
        torch.cuda.synchronize()
        assert guarded.intact(), "a guard band around the scratch buffer was written"
        return row, torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    row, grad = step()
    assert np.isfinite(row).all() and np.isfinite(grad).all()
    ref = I.regae_oracle(c, inp, torch.float64)
    errs, e32 = I.regae_errors(c, row, grad.astype(np.float64), ref[0], ref[1]), I.regae_e32(c, inp, ref)
    ERRORS[c.id] = dict(group="regae", **{t: errs[t] for t in A.REGAE_TERMS}, **{"e32_" + t: e32[t] for t in A.REGAE_TERMS})
    print(c.id + ": " + ", ".join(f"{t} {errs[t]:.1e} (e32 {e32[t]:.1e})" for t in A.REGAE_TERMS))
    for t in A.REGAE_TERMS:
        assert errs[t] <= A.REGAE_BARS[t], f"{t}: {errs[t]:.2e} > {A.REGAE_BARS[t]:.2e} (fp32 oracle: {e32[t]:.2e})"
    assert row[4 + c.K] == 0.0                                   # the gradient-norm term is off

    row_again, grad_again = step()
    assert row_again.tobytes() == row.tobytes() and grad_again.tobytes() == grad.tobytes(), "two steps on the same inputs differ"

    if c.handoff:   # forward_keep / backward_reuse against forward / backward
        plain = _PlainPair(_hip.lib())
        monkeypatch.setattr(_hip, "lib", lambda: plain)
        row_p, grad_p = step()
        monkeypatch.undo()
        assert row_p.tobytes() == row.tobytes() and grad_p.tobytes() == grad.tobytes(), "the hand-off changes the step's bits"

    if c.dup:
        assert A.regae_grid(c)[1] == 2 and A.regae_grid(c, 2)[1] > 2 and c.B % A.TILE
        row2, grad2 = step(2)
        errs2 = I.regae_errors(c, row2, grad2.astype(np.float64), ref[0], ref[1])
        ERRORS[c.id].update({"dup_" + t: errs2[t] for t in A.REGAE_TERMS})
        for t in A.REGAE_TERMS:
            assert errs2[t] <= A.REGAE_BARS[t], f"two copies, {t}: {errs2[t]:.2e} > {A.REGAE_BARS[t]:.2e}"
        np.testing.assert_allclose(row2, row, rtol=DUP_TOL["loss"], atol=1e-12)
        np.testing.assert_allclose(grad2, grad, rtol=DUP_TOL["grad"], atol=DUP_TOL["grad_abs"] * np.abs(grad).max())
