"""GPU (-m gpu): bias energy and forces along a CV in one launch, in an MD engine's arrays (cvf_cv_frame_bias_eval and its _large /
_shared forms, csrc/cv_bias.hip) and export.BiasedCV.  Models, bias cases, the independent fp64 bias and the bars:
tests/cv_bias_cases.py.  Every check runs on both kernels and on forms A, B and C, B = 3 different frames.

  bits     xi_rows and the force added to a zero-filled dense F_all are the namesake's (cvf_cv_frame[_large][_shared]_eval with
           coef = -du_rows), torch.equal: the new path is tied to kernels already tested against fp64
  layout   N_total = n_atoms + 5 engine atoms of 4 floats, a shuffled atom_index, frame strides past the frame and different for x
           and f; X_all is NaN wherever the launch must not read, F_all random wherever it must not write
  fp64     U, dU and the force against torch fp64 autograd of U(xi(x)); measured on the MI355X: DESIGN.md section 4.18"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cv_bias_cases as Bc

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


_SETUPS = {}


def setup(dev, mid):
    """Everything a model needs, built once: descriptors, theta and frames on the device, the entry points of its kernel and form,
    and xi0 - what the namesake gives for the frames (the bias cases are placed around it)."""
    if mid in _SETUPS:
        return _SETUPS[mid]
    from colvarsfinder import _hip
    from colvarsfinder.pp import identity_desc
    lib = _hip.lib()
    layer = Bc.hip_layer(mid, dev)
    nets = Bc.nets_of(mid)
    mdesc, cut, k, theta, ns = Bc.plan_of(nets)
    frames = Bc.model_parts(mid)[4]
    x = torch.tensor(frames, device=dev).reshape(Bc.B, -1).contiguous()
    pdesc = identity_desc(x.shape[1]) if isinstance(layer, torch.nn.Identity) else layer.pp_desc()
    name = "cvf_cv_frame" + ("_large" if mid.startswith("large") else "")
    sh = "_shared" if ns > 0 else ""
    s = dict(mid=mid, layer=layer, nets=nets, mdesc=mdesc, cut=cut, k=k, theta=theta.to(dev), pdesc=pdesc, x=x, frames=frames, n=x.shape[1],
             plain=getattr(lib, name + sh + "_eval"), bias=getattr(lib, name + "_bias" + sh + "_eval"),
             plain_ok=getattr(lib, name + sh + "_supported"), bias_ok=getattr(lib, name + "_bias" + sh + "_supported"))
    assert s["plain_ok"](mdesc, cut, pdesc) == 1 and s["bias_ok"](mdesc, cut, pdesc) == 1, lib.cvf_last_error().decode()
    s["xi0"], _ = namesake(s, x)
    _SETUPS[mid] = s
    return s


def namesake(s, x, coef=None):
    """(xi [B, k], gx) of the model's cvf_cv_frame[_large][_shared]_eval."""
    from colvarsfinder import _hip
    P = _hip.ptr
    B, k, n = x.shape[0], s["k"], s["n"]
    xi = torch.full((B, k), NAN, device=x.device)
    gx = torch.full((B, n) if coef is not None else (B, k, n), NAN, device=x.device)
    rc = s["plain"](s["mdesc"], P(s["theta"]), s["cut"], s["pdesc"], P(x), B, P(coef), P(xi), P(gx), _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, _hip.lib().cvf_last_error().decode()
    return xi, gx


def bias_call(s, desc, X_all, F_all, B, layout=None, want_du=True):
    """(rc, xi [B, k], U [B], dU [B, k]) of the model's bias entry point; the three outputs start as NaN, F_all is the caller's."""
    from colvarsfinder import _hip
    P = _hip.ptr
    k, dev = s["k"], X_all.device
    xi, U, dU = torch.full((max(B, 1), k), NAN, device=dev), torch.full((max(B, 1),), NAN, device=dev), torch.full((max(B, 1), k), NAN, device=dev)
    rc = s["bias"](s["mdesc"], P(s["theta"]), s["cut"], s["pdesc"], desc, layout, C.c_void_p(X_all.data_ptr()), B, P(xi), P(U),
                   P(dU) if want_du else None, C.c_void_p(F_all.data_ptr()), _hip.stream())
    torch.cuda.synchronize()
    return rc, xi[:B], U[:B], dU[:B]


def bias_of(s, case, dev):
    """(terms, BiasDesc, table tensor) of a bias case placed around the model's xi0."""
    from colvarsfinder import export
    terms = Bc.terms_for(case, s["xi0"].cpu().numpy())
    desc, table = export.bias_desc(terms, s["k"], dev)
    return terms, desc, table


def dense(s, desc):
    """(xi, U, dU, F [B, n]) of the bias launch on the dense layout over a zero-filled F."""
    F = torch.zeros_like(s["x"])
    rc, xi, U, dU = bias_call(s, desc, s["x"], F, Bc.B)
    assert rc == 0
    return xi, U, dU, F


ALL_MODELS = Bc.MODELS_WAVE + Bc.MODELS_LARGE


@pytest.mark.parametrize("case", ["three-on-one", "table"])
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_bits_are_the_namesakes(dev, mid, case):
    s = setup(dev, mid)
    _, desc, table = bias_of(s, case, dev)
    xi, U, dU, F = dense(s, desc)
    assert not torch.isnan(xi).any() and not torch.isnan(U).any() and not torch.isnan(dU).any() and not torch.isnan(F).any()
    assert torch.equal(xi, s["xi0"])
    _, Fn = namesake(s, s["x"], coef=(-dU).contiguous())
    assert torch.equal(F, Fn)
    assert (dU != 0).any() and (F != 0).any()
    # du_rows may be NULL: the same bits
    F2 = torch.zeros_like(F)
    rc, xi2, U2, _ = bias_call(s, desc, s["x"], F2, Bc.B, want_du=False)
    assert rc == 0 and torch.equal(F2, F) and torch.equal(U2, U) and torch.equal(xi2, xi)


def engine_arrays(s, dev, seed):
    """An engine's view of the model's frames: (X_all [B, xs], F_all [B, fs] random, layout, atom_index, cols [n] - the float of
    coordinate j inside a frame).  X_all is NaN on every float that is not a coordinate of a CV atom."""
    from colvarsfinder import _hip
    n = s["n"]
    assert n % 3 == 0
    n_atoms, stride = n // 3, 4
    n_total = n_atoms + 5
    g = torch.Generator().manual_seed(seed)
    index = torch.randperm(n_total, generator=g)[:n_atoms].to(torch.int32)
    xs, fs = n_total * stride + 7, n_total * stride + 13
    a = torch.arange(n)
    cols = (index.long()[a // 3] * stride + a % 3).to(dev)
    X_all = torch.full((Bc.B, xs), NAN, device=dev)
    X_all[:, cols] = s["x"]
    F_all = torch.randn(Bc.B, fs, generator=g).to(dev)
    index = index.to(dev)
    layout = _hip.MDLayout(index.data_ptr(), stride, 0, xs, fs)
    return X_all, F_all, layout, index, cols


@pytest.mark.parametrize("mid", ALL_MODELS)
def test_engine_layout(dev, mid):
    s = setup(dev, mid)
    _, desc, table = bias_of(s, "three-on-one", dev)
    xi_d, U_d, dU_d, F_d = dense(s, desc)
    X_all, F_all, layout, index, cols = engine_arrays(s, dev, seed=len(mid))
    before = F_all.clone()
    rc, xi, U, dU = bias_call(s, desc, X_all, F_all, Bc.B, layout)
    assert rc == 0
    assert torch.equal(xi, xi_d) and torch.equal(U, U_d) and torch.equal(dU, dU_d)      # (nothing outside the CV's atoms was read: no NaN)
    touched = torch.zeros_like(F_all, dtype=torch.bool)
    touched[:, cols] = True
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32))   # other atoms, padding floats, gaps
    assert torch.equal(F_all[:, cols], before[:, cols] + F_d)                             # fp32(before + dense result)
    # a second identical call adds the same amount again
    once = F_all.clone()
    rc, _, _, _ = bias_call(s, desc, X_all, F_all, Bc.B, layout)
    assert rc == 0 and torch.equal(F_all[:, cols], once[:, cols] + F_d)
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32))
    # frame b alone (B = 1) gives frame b's bits
    for b in range(Bc.B):
        F1 = before[b:b + 1].clone()
        rc, xi1, U1, dU1 = bias_call(s, desc, X_all[b:b + 1].contiguous(), F1, 1, layout)
        assert rc == 0 and torch.equal(xi1[0], xi[b]) and torch.equal(U1[0], U[b]) and torch.equal(dU1[0], dU[b])
        assert torch.equal(F1[0], once[b]), b
    # x_all is only read: x_frame_stride = 0 gives every replica frame 0
    from colvarsfinder import _hip
    F0 = before.clone()
    rc, xib, _, _ = bias_call(s, desc, X_all, F0, Bc.B, _hip.MDLayout(index.data_ptr(), 4, 0, 0, layout.f_frame_stride))
    assert rc == 0 and all(torch.equal(xib[b], xi[0]) for b in range(Bc.B)) and torch.equal(F0[0], once[0])


def test_layout_without_an_index_and_identity_frames_of_any_length(dev):
    """atom_index = NULL is the identity map under the stride; the CVF_PP_IDENTITY model (n_coord = 6) through both."""
    from colvarsfinder import _hip
    for mid in ("wave-identity", "large-B"):
        s = setup(dev, mid)
        _, desc, table = bias_of(s, "harmonic", dev)
        _, U_d, _, F_d = dense(s, desc)
        n, stride = s["n"], 5
        a = torch.arange(n, device=dev)
        cols = a // 3 * stride + a % 3
        xs = fs = (n // 3) * stride
        X_all = torch.full((Bc.B, xs), NAN, device=dev)
        X_all[:, cols] = s["x"]
        F_all = torch.ones(Bc.B, fs, device=dev)
        rc, _, U, _ = bias_call(s, desc, X_all, F_all, Bc.B, _hip.MDLayout(None, stride, 0, xs, fs))
        assert rc == 0 and torch.equal(U, U_d) and torch.equal(F_all[:, cols], 1.0 + F_d)
        rest = torch.ones_like(F_all, dtype=torch.bool)
        rest[:, cols] = False
        assert (F_all[rest] == 1.0).all()


@pytest.mark.parametrize("case", Bc.BIAS_CASES)
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_against_fp64_autograd(dev, mid, case):
    s = setup(dev, mid)
    terms, desc, table = bias_of(s, case, dev)
    xi, U, dU, F = dense(s, desc)
    U64, dU64, F64 = Bc.reference(mid, s["nets"], s["frames"], terms)
    eu, ed, ef = Bc.rel_rows(U.cpu().numpy(), U64), Bc.rel_rows(dU.cpu().numpy(), dU64), Bc.rel_rows(F.cpu().numpy(), F64)
    print(f"[cvbias] {mid} {case}: U {eu:.2e} dU {ed:.2e} force {ef:.2e}")
    assert np.isfinite(F64).all() and np.abs(F64).max() > 1e-3
    assert eu <= Bc.U_TOL and ed <= Bc.DU_TOL and ef <= Bc.F_TOL
    if case.startswith("table"):      # the three frames fall below lo, inside an inner interval and above the last node
        t = terms[0]
        sidx = np.sort((s["xi0"][:, 0].cpu().numpy().astype(np.float64) - np.float32(t["lo"])) * np.float32(t["inv_h"]))
        assert sidx[0] < 0 and 1 <= sidx[1] <= 3 and sidx[2] > len(t["u"]) - 1, sidx
    if case == "table-node-at-xi":
        assert sidx[1] == 2.0


def test_refusals_leave_everything_untouched(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import identity_desc
    from tests import cv_frame_cases as Fc
    lib = _hip.lib()
    for mid in ("wave-A", "large-C"):
        s = setup(dev, mid)
        _, good, table = bias_of(s, "table", dev)
        X_all, F_all, layout, index, cols = engine_arrays(s, dev, seed=3)
        before = F_all.clone()
        bad_cv, bad_table = _hip.BiasDesc.from_buffer_copy(good), _hip.BiasDesc.from_buffer_copy(good)
        bad_cv.term[0].cv = s["k"]
        bad_table.n_table -= 1
        stride2 = _hip.MDLayout(index.data_ptr(), 2, 0, layout.x_frame_stride, layout.f_frame_stride)
        # force frames that overlap: two workgroups would accumulate into the same floats (a repeated x frame is only read, and fine)
        overlap = _hip.MDLayout(index.data_ptr(), 4, 0, layout.x_frame_stride, 0)
        short = _hip.MDLayout(index.data_ptr(), 4, 0, 0, (s["n"] // 3 - 1) * 4 + 2)
        for name, desc, lay, words in (("cv == k", bad_cv, layout, "term[0].cv"), ("table overrun", bad_table, layout, "n_table"),
                                       ("atom_stride = 2", good, stride2, "atom_stride = 2"), ("f_frame_stride = 0", good, overlap, "f_frame_stride = 0"),
                                       ("f_frame_stride short", good, short, "f_frame_stride")):
            rc, xi, U, dU = bias_call(s, desc, X_all, F_all, Bc.B, lay)
            why = lib.cvf_last_error().decode()
            assert rc < 0 and words in why, (name, rc, why)
            assert torch.isnan(xi).all() and torch.isnan(U).all() and torch.isnan(dU).all(), name
            assert torch.equal(F_all.view(torch.int32), before.view(torch.int32)), name
        # an empty batch is no error and writes nothing
        rc, xi, U, dU = bias_call(s, good, X_all, F_all, 0, layout)
        assert rc == 0 and torch.isnan(xi).all() and torch.isnan(U).all() and torch.equal(F_all.view(torch.int32), before.view(torch.int32))
    # an atom index over identity frames that are no whole atoms
    m, pdesc, theta = Fc.mlp([4, 5, 1], 2), identity_desc(4), torch.zeros(64, device=dev)
    assert lib.cvf_cv_frame_bias_supported(m, 2, pdesc) == 1
    empty = _hip.BiasDesc()
    x4, f4, xi, U = torch.zeros(1, 8, device=dev), torch.full((1, 8), 2.0, device=dev), torch.full((1, 2), NAN, device=dev), torch.full((1,), NAN, device=dev)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    rc = lib.cvf_cv_frame_bias_eval(m, _hip.ptr(theta), 2, pdesc, empty, _hip.MDLayout(idx.data_ptr(), 3, 0, 8, 8), _hip.ptr(x4), 1, _hip.ptr(xi),
                                    _hip.ptr(U), None, _hip.ptr(f4), _hip.stream())
    torch.cuda.synchronize()
    why = lib.cvf_last_error().decode()
    assert rc < 0 and "CVF_PP_IDENTITY" in why and "n_coord = 4" in why, why
    assert torch.isnan(xi).all() and torch.isnan(U).all() and (f4 == 2.0).all()


# ------------------------------------------------------------------------------------------------ export.BiasedCV
def cv_model(mid, dev):
    from colvarsfinder import core
    s = setup(dev, mid)
    cv = core._CVModel(s["layer"], s["nets"].to(dev), device=dev)
    cv.shared_trunk = type(s["nets"]).__name__ == "SharedEigenFunctions"
    return s, cv


@pytest.mark.parametrize("mid,large,route", [("wave-A", False, "frame"), ("wave-C", False, "frame"), ("large-A-weighted", True, "frame-large"),
                                             ("large-C", True, "frame-large")])
def test_biased_cv_one_launch_routes(dev, mid, large, route):
    from colvarsfinder import export
    s, cv = cv_model(mid, dev)
    terms = Bc.terms_for("table", s["xi0"].cpu().numpy())
    X_all, F_all, layout, index, cols = engine_arrays(s, dev, seed=11)
    n_total = s["n"] // 3 + 5
    bc = export.BiasedCV(cv, terms, dev, large_frames=large, atom_index=index.cpu(), atom_stride=4)
    assert bc.route == route and bc.table.is_cuda
    engine = lambda T: T[:, :n_total * 4].view(Bc.B, n_total, 4)      # (a view: the frame strides stay past the frame)
    # into a zero-filled force array: the force itself, against fp64 within the bars
    F_zero = torch.zeros_like(F_all)
    xi, U, dU = bc(engine(X_all), engine(F_zero))
    force = F_zero[:, cols].clone()
    U64, dU64, F64 = Bc.reference(mid, s["nets"], s["frames"], terms)
    eu, ed, ef = Bc.rel_rows(U.cpu().numpy(), U64), Bc.rel_rows(dU.cpu().numpy(), dU64), Bc.rel_rows(force.cpu().numpy(), F64)
    print(f"[cvbias] BiasedCV {mid} {bc.route}: U {eu:.2e} dU {ed:.2e} force {ef:.2e}")
    assert eu <= Bc.U_TOL and ed <= Bc.DU_TOL and ef <= Bc.F_TOL and torch.equal(xi, s["xi0"])
    F_zero[:, cols] = 0.0
    assert (F_zero == 0).all()
    # into the engine's random forces: fp32(before + that force) on the CV's atoms, every other bit kept
    before = F_all.clone()
    xi2, U2, dU2 = bc(engine(X_all), engine(F_all))
    assert torch.equal(xi2, xi) and torch.equal(U2, U) and torch.equal(dU2, dU)
    assert torch.equal(F_all[:, cols], before[:, cols] + force)
    before[:, cols] = F_all[:, cols]
    assert torch.equal(F_all.view(torch.int32), before.view(torch.int32))
    # the table is read at launch time: scaled in place, the table term's energy and force scale with it
    only_table = [terms[0]]
    bt = export.BiasedCV(cv, only_table, dev, large_frames=large)
    f1, f2 = torch.zeros_like(s["x"]), torch.zeros_like(s["x"])
    _, U1, dU1 = bt(s["x"], f1)
    bt.table.mul_(2.0)
    _, U2, dU2 = bt(s["x"], f2)
    assert torch.equal(U2, 2.0 * U1) and torch.equal(dU2, 2.0 * dU1) and torch.equal(f2, 2.0 * f1) and (f1 != 0).any()
    with pytest.raises(ValueError, match="cv = 2"):
        export.BiasedCV(cv, [("harmonic", 2, 1.0, 0.0)], dev)
    with pytest.raises(ValueError, match="distinct"):
        export.BiasedCV(cv, terms, dev, atom_index=[0] * (s["n"] // 3))


def test_biased_cv_three_call_route_agrees(dev):
    """mixed65 (tests/test_align_vjp_gpu.case) under nets 300 wide - no entry of the case tables is past BOTH launches, so this one
    is built here: large_frames=True still ends on the three-call route, checked against the fp64 autograd of the same bias."""
    from colvarsfinder import core, export, nn
    from tests import cv_frame_large_cases as G
    from tests.test_cv_jacobian_gpu import layer_of
    layer, traj, ref = layer_of("mixed65", Bc.B, False, dev)
    torch.manual_seed(8)
    nets = nn.EigenFunctions([layer.d_r, 300, 1], 2)
    cv = core._CVModel(layer, nets.to(dev), device=dev)
    x = torch.tensor(traj, device=dev).reshape(Bc.B, -1).contiguous()
    xi0, _ = export.FrameCV(cv, dev, large_frames=True)(x)
    terms = Bc.terms_for("table", xi0.cpu().numpy()) + [{"kind": "upper_wall", "cv": 1, "kappa": 1.2, "center": float(xi0[:, 1].median())}]
    bc = export.BiasedCV(cv, terms, dev, large_frames=True)
    assert bc.route == "three-call" and "300 wide" in bc.supported[1] and "300 wide" in bc.supported_large[1]
    F = torch.zeros_like(x)
    xi, U, dU = bc(x, F)
    # fp64 autograd through the oracle's layer
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    pp64 = G.torch_layer("mixed65", torch.float64)
    import copy
    xi64 = copy.deepcopy(nets).to("cpu", torch.float64)(pp64(X)).reshape(Bc.B, -1)
    U64 = Bc.ref_bias(terms, xi64)
    U64.sum().backward()
    eu, ef = Bc.rel_rows(U.cpu().numpy(), U64.detach().numpy()), Bc.rel_rows(F.cpu().numpy(), -X.grad.reshape(Bc.B, -1).numpy())
    print(f"[cvbias] BiasedCV mixed65 x 300 three-call: U {eu:.2e} force {ef:.2e}")
    assert eu <= Bc.U_TOL and ef <= Bc.F_TOL


def test_biased_cv_routes_agree_on_a_case_table_model(dev):
    """("mixed65", "A-k3") of tests/cv_frame_large_cases.LAYER_CASES: the wave launch declines its 65 atoms, so the default
    BiasedCV takes the three calls and large_frames=True the workgroup launch - each against fp64 and against the other, all
    within the bars."""
    import copy
    from colvarsfinder import core, export
    from tests import cv_frame_large_cases as G
    layer, nets = G.hip_layer("mixed65", dev), G.nets_for("mixed65", "A-k3")
    traj, _ = G.frames("mixed65")
    assert traj.shape[0] == Bc.B
    cv = core._CVModel(layer, copy.deepcopy(nets).to(dev), device=dev)
    x = torch.tensor(traj, device=dev).reshape(Bc.B, -1).contiguous()
    xi0, _ = export.FrameCV(cv, dev)(x)
    terms = Bc.terms_for("three-on-one", xi0.cpu().numpy()) + [{"kind": "harmonic", "cv": 2, "kappa": 0.9, "center": float(xi0[:, 2].min() - 1.5)}]
    three, large = export.BiasedCV(cv, terms, dev), export.BiasedCV(cv, terms, dev, large_frames=True)
    assert three.route == "three-call" and "n_coord = 195" in three.supported[1] and large.route == "frame-large"
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    xi64 = copy.deepcopy(nets).to("cpu", torch.float64)(G.torch_layer("mixed65", torch.float64)(X)).reshape(Bc.B, -1)
    U64 = Bc.ref_bias(terms, xi64)
    U64.sum().backward()
    U64, F64 = U64.detach().numpy(), -X.grad.reshape(Bc.B, -1).numpy()
    out = {}
    for name, bc in (("three-call", three), ("frame-large", large)):
        F = torch.zeros_like(x)
        _, U, _ = bc(x, F)
        out[name] = (U.cpu().numpy(), F.cpu().numpy())
        eu, ef = Bc.rel_rows(out[name][0], U64), Bc.rel_rows(out[name][1], F64)
        print(f"[cvbias] BiasedCV mixed65 A-k3 {name}: U {eu:.2e} force {ef:.2e}")
        assert eu <= Bc.U_TOL and ef <= Bc.F_TOL
    d_u, d_f = Bc.rel_rows(out["three-call"][0], out["frame-large"][0]), Bc.rel_rows(out["three-call"][1], out["frame-large"][1])
    print(f"[cvbias] BiasedCV mixed65 A-k3 three-call against frame-large: U {d_u:.2e} force {d_f:.2e}")
    assert d_u <= Bc.U_TOL and d_f <= Bc.F_TOL
