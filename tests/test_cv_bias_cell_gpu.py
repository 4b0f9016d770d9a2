"""GPU (-m gpu): periodic cells in the bias launches - whole molecules and the virial (cvf_cv_frame[_large]_bias[_shared]_cell_eval,
cvf_md_make_whole, csrc/cv_bias.hip; the rule: csrc/cvf_cell.hpp) and export.BiasedCV / export.make_whole.
The eight models of tests/cv_bias_cases.py x three cells (and one batch whose cell differs per frame) x two bias cases, B = 3.

  frames   the models' frames torn under the cell: frame 0 with every atom wrapped into the cell and moved by a random lattice vector
           (breaks everywhere, inside the aligned atoms too), frame 1 with one break between an aligned atom and one that is not,
           frame 2 whole.  The cells are the host tests' scaled by a power of two to the molecule (consecutive atoms within 0.4 of the
           shortest height), with dyadic off-diagonal entries: every N h is exact in fp32, so the whole positions carry no more
           rounding than the frames themselves and the standing bars against fp64 apply
  layout   the shuffled 4-float one with 5 extra engine atoms, X_all NaN wherever it must not be read
  bits     cvf_md_make_whole against the host program tools/cell_host.cpp (built here WITHOUT sanitizers: the CPU tests run it under
           them and compare the two builds); the four _cell_eval launches against their namesakes on cvf_md_make_whole's dense output
  fp64     the sequential rule in numpy, then torch autograd of U(xi(.)): the bars of tests/cv_bias_cases.py and cv_bias2_cases.py
  virial   against d U(xi((I + eps) r_whole)) / d eps at 0 by fp64 autograd; measured on the MI355X: V_TOL below"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cv_bias2_cases as B2
from tests import cv_bias_cases as Bc
from tests import cv_cell_cases as Cc
from tests import test_cv_bias_gpu as T1

pytestmark = pytest.mark.gpu
NAN = float("nan")
dev = T1.dev

# The virial's bar (metric: max abs error over the 9 entries / sum_a |r_a| |f_a|, the largest over the frames; reference: fp64 autograd
# in the strain).  Three times the worst measured on the MI355X over all (model, cell, case) triples; figures in DESIGN.md 4.20.
V_TOL = 1.24e-6    # achieved 4.12e-7 (wave-C, orthorhombic, grid); 3.1e-8 .. 4.1e-7 over the 64 triples; torch fp32 of the launch's outputs: 2.3e-8 .. 4.1e-7

# the virial, route against route (three-call: torch fp32 of the dense arrays; frame-large: the launch), max abs difference / the largest
# entry: three times the 2.65e-7 measured on the MI355X, as the bars of 4.18 were set
V_ROUTE_TOL = 8.0e-7

CELL_NAMES = ["ortho", "dyadic", "slab", "per-frame"]
BASE = {"ortho": Cc.ORTHO, "dyadic": Cc.DYADIC, "slab": Cc.SLAB, "triclinic": Cc.TRICLINIC}
# the bit-for-bit checks also run on the host test's triclinic cell, whose lattice shifts are NOT exact in fp32: there the order of the
# shift's sum, every fused multiply-add and a contracted x - N.z cz would each show in the last bit (no fp64 bar is involved)
BITS_CELLS = CELL_NAMES + ["triclinic"]
CASES = ["harmonic", "grid"]


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return Cc.build_program(tmp_path_factory.mktemp("cell_gpu"), sanitize=False)


def scaled_cells(frames3, name):
    """[B, 9] fp32 cells for whole frames [B, n, 3]: the base cells times the power of two that keeps consecutive atoms within 0.4 of
    the shortest height; "per-frame": another cell and another scale for every frame."""
    d = np.abs(np.diff(frames3.astype(np.float64), axis=1)).max() if frames3.shape[1] > 1 else 1.0
    s = 2.0 ** np.ceil(np.log2(2.5 * d / 2.0))
    B = frames3.shape[0]
    if name == "per-frame":
        kinds = ["dyadic", "slab", "ortho"]
        return np.stack([BASE[kinds[b % 3]] * s * 2.0 ** b for b in range(B)]).astype(np.float32)
    return np.stack([BASE[name] * s] * B).astype(np.float32)


def break_index(n_atoms, align):
    """An atom j with exactly one of j - 1, j among the align atoms (no alignment: the middle atom)."""
    if align is None:
        return max(1, n_atoms // 2)
    a = set(align)
    return next(j for j in range(max(1, n_atoms // 2), n_atoms) if (j in a) != (j - 1 in a))


def torn_frames(frames3, cells, align, seed):
    """fp32 [B, n, 3]: frame 0 wrapped and shifted atom by atom, frame 1 with one break, the others whole."""
    rs = np.random.RandomState(seed)
    out = frames3.astype(np.float32).copy()
    out[0] = Cc.tear(cells[0], frames3[0], rs, shifts=2, keep_first=True, centred=True)
    if len(out) > 1:
        out[1] = Cc.break_at(cells[1], frames3[1], break_index(frames3.shape[1], align), (1, -1, 2))
    return out


def engine_arrays(x, dev, seed):
    """tests/test_cv_bias_gpu.engine_arrays for the frames x [B, n] (a device tensor): (X_all, F_all, layout, index, cols)."""
    from colvarsfinder import _hip
    B, n = x.shape
    n_atoms, stride = n // 3, 4
    n_total = n_atoms + 5
    g = torch.Generator().manual_seed(seed)
    index = torch.randperm(n_total, generator=g)[:n_atoms].to(torch.int32)
    xs, fs = n_total * stride + 7, n_total * stride + 13
    a = torch.arange(n)
    cols = (index.long()[a // 3] * stride + a % 3).to(dev)
    X_all = torch.full((B, xs), NAN, device=dev)
    X_all[:, cols] = x
    F_all = torch.randn(B, fs, generator=g).to(dev)
    index = index.to(dev)
    return X_all, F_all, _hip.MDLayout(index.data_ptr(), stride, 0, xs, fs), index, cols


def make_whole(X_all, layout, cell_t, stride, n_atoms, B, out=None):
    from colvarsfinder import _hip
    out = torch.full((B, 3 * n_atoms), NAN, device=X_all.device) if out is None else out
    mc = _hip.MDCell(cell_t.data_ptr(), stride, None)
    rc = _hip.lib().cvf_md_make_whole(layout, mc, C.c_void_p(X_all.data_ptr()), n_atoms, B, C.c_void_p(out.data_ptr()), _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, _hip.lib().cvf_last_error().decode()
    return out


def cell_call(s, desc, X_all, F_all, B, layout, mc, want_du=True):
    """(rc, xi, U, dU) of the model's _cell_eval; the three outputs start as NaN."""
    from colvarsfinder import _hip
    P = _hip.ptr
    k, d = s["k"], X_all.device
    name = "cvf_cv_frame" + ("_large" if s["mid"].startswith("large") else "") + "_bias" + ("_shared" if s["mid"].endswith("-C") else "") + "_cell_eval"
    xi, U, dU = torch.full((max(B, 1), k), NAN, device=d), torch.full((max(B, 1),), NAN, device=d), torch.full((max(B, 1), k), NAN, device=d)
    rc = getattr(_hip.lib(), name)(s["mdesc"], P(s["theta"]), s["cut"], s["pdesc"], desc, layout, C.c_void_p(X_all.data_ptr()), B, P(xi), P(U),
                                   P(dU) if want_du else None, C.c_void_p(F_all.data_ptr()), _hip.stream(), mc)
    torch.cuda.synchronize()
    return rc, xi[:B], U[:B], dU[:B]


def terms_of(s, case):
    xi0 = s["xi0"].cpu().numpy()
    if case == "harmonic":
        return Bc.terms_for("harmonic", xi0), (Bc.U_TOL, Bc.DU_TOL, Bc.F_TOL)
    return B2.grid_terms("interior", xi0), (B2.U_TOL, B2.DU_TOL, B2.F_TOL)


_WORLD = {}


def world(dev, mid, cname):
    """The torn frames of a model under a cell configuration in the engine's arrays, and their whole forms: made once."""
    key = (mid, cname)
    if key in _WORLD:
        return _WORLD[key]
    s = T1.setup(dev, mid)
    n = s["n"]
    frames3 = np.asarray(s["frames"], dtype=np.float32).reshape(Bc.B, n // 3, 3)
    cells = scaled_cells(frames3, cname)
    torn = torn_frames(frames3, cells, Bc.model_parts(mid)[1], seed=len(mid) + len(cname))
    w64 = np.stack([Cc.whole_fp64(cells[b], torn[b])[0] for b in range(Bc.B)])
    for b in range(Bc.B):
        assert Cc.whole_fp64(cells[b], torn[b])[2] >= 0.05           # far from a half-integer: the precondition holds with room
    x = torch.tensor(torn.reshape(Bc.B, n), device=dev)
    X_all, F_all, layout, index, cols = engine_arrays(x, dev, seed=len(mid) + 3)
    per_frame = cname == "per-frame"
    cell_t = torch.tensor(cells if per_frame else cells[0], device=dev).contiguous()
    stride = 9 if per_frame else 0
    xw = make_whole(X_all, layout, cell_t, stride, n // 3, Bc.B)
    w = dict(s=s, cells=cells, torn=torn, w64=w64, X_all=X_all, F_all=F_all, layout=layout, index=index, cols=cols, cell_t=cell_t,
             stride=stride, xw=xw)
    _WORLD[key] = w
    return w


ALL_MODELS = Bc.MODELS_WAVE + Bc.MODELS_LARGE


@pytest.mark.parametrize("cname", BITS_CELLS)
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_make_whole_is_the_host_programs(dev, program, mid, cname):
    w = world(dev, mid, cname)
    n = w["s"]["n"]
    N, W, _ = program(w["cells"], w["torn"])
    got = w["xw"].cpu().numpy().reshape(Bc.B, n // 3, 3)
    assert np.array_equal(got.view(np.uint32), W.view(np.uint32))
    assert (N[0] != 0).any() and (N[1] != 0).any() and (N[2] == 0).all()
    assert np.array_equal(got[2].view(np.uint32), w["torn"][2].view(np.uint32))        # the whole frame: bit for bit
    N64 = np.stack([Cc.whole_fp64(w["cells"][b], w["torn"][b])[1] for b in range(Bc.B)])
    assert np.array_equal(N, N64)
    inexact = 0
    for b in range(Bc.B):
        x64, h = w["torn"][b].astype(np.float64), Cc.lattice(w["cells"][b])
        if cname != "triclinic":   # the shifts of these cells are exact in fp32: one rounding, of the exact difference
            assert np.array_equal(got[b].view(np.uint32), (x64 - N64[b] @ h).astype(np.float32).view(np.uint32)), b
        else:                      # within the derived bound, and the shifts really round
            assert (np.abs(got[b].astype(np.float64) - w["w64"][b]) <= 4 * Cc.EPS * (np.abs(x64) + np.abs(N64[b]) @ np.abs(h))).all(), b
            inexact += int(((N64[b] @ h).astype(np.float32).astype(np.float64) != N64[b] @ h).sum())
    assert cname != "triclinic" or inexact > 0
    # the output is dense [B][3 n_atoms]: nothing behind it is written
    out = torch.full((Bc.B * n + 64,), 7.5, device=dev)
    make_whole(w["X_all"], w["layout"], w["cell_t"], w["stride"], n // 3, Bc.B, out=out)
    assert torch.equal(out[:Bc.B * n].view(Bc.B, n), w["xw"]) and (out[Bc.B * n:] == 7.5).all()


@pytest.mark.parametrize("n_atoms", [257, 513])
def test_chunk_carry_of_the_stand_alone_and_workgroup_scans(dev, program, n_atoms):
    """More atoms than a chunk of 256: the carried totals of cvf_md_make_whole against the host program, and the workgroup kernel's
    prologue against its namesake on that output, bit for bit."""
    from colvarsfinder import _hip, nn, pp
    from tests.synth import make_molecule_traj
    traj, _, ref = make_molecule_traj(n_atoms, Bc.B, seed=n_atoms, sigma=0.8)
    cells = scaled_cells(traj, "triclinic")          # (shifts that round in fp32: the bits also check the form of the subtraction)
    rs = np.random.RandomState(n_atoms)
    torn = np.stack([Cc.tear(cells[b], traj[b], rs, shifts=2, keep_first=True, centred=True) for b in range(Bc.B)])
    x = torch.tensor(torn.reshape(Bc.B, -1), device=dev)
    X_all, F_all, layout, index, cols = engine_arrays(x, dev, seed=n_atoms)
    cell_t = torch.tensor(cells[0], device=dev)
    xw = make_whole(X_all, layout, cell_t, 0, n_atoms, Bc.B)
    N, W, _ = program(cells, torn)
    assert np.array_equal(xw.cpu().numpy().reshape(Bc.B, n_atoms, 3).view(np.uint32), W.view(np.uint32))
    assert (N[:, 256:] != 0).any() and np.abs(N).max() >= 2
    # the workgroup kernel on a model of that many atoms
    align = [a for a in range(n_atoms) if a % 7 not in (0, 4)]
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], Bc.spread(Bc.FEATS7, 7, n_atoms), False).to(dev)
    torch.manual_seed(n_atoms)
    nets = nn.EigenFunctions([layer.d_r, 5, 1], 2, activation=torch.nn.Tanh())
    mdesc, cut, k, theta, ns = Bc.plan_of(nets)
    lib = _hip.lib()
    s = dict(mid="large-A", mdesc=mdesc, cut=cut, k=k, theta=theta.to(dev), pdesc=layer.pp_desc(), n=3 * n_atoms,
             bias=lib.cvf_cv_frame_large_bias_eval)
    from colvarsfinder import export
    desc, table = export.bias_desc([{"kind": "harmonic", "cv": 0, "kappa": 1.3, "center": -1.0}, {"kind": "harmonic", "cv": 1, "kappa": 0.8, "center": 1.0}], 2, dev)
    F_d = torch.zeros_like(xw)
    rc, xi_d, U_d, dU_d = T1.bias_call(s, desc, xw, F_d, Bc.B)
    assert rc == 0, lib.cvf_last_error().decode()
    vir = torch.full((Bc.B, 9), NAN, device=dev)
    before = F_all.clone()
    rc, xi, U, dU = cell_call(s, desc, X_all, F_all, Bc.B, layout, _hip.MDCell(cell_t.data_ptr(), 0, vir.data_ptr()))
    assert rc == 0, lib.cvf_last_error().decode()
    assert torch.equal(xi, xi_d) and torch.equal(U, U_d) and torch.equal(dU, dU_d) and (F_d != 0).any()
    assert torch.equal(F_all[:, cols], before[:, cols] + F_d) and not torch.isnan(vir).any()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cname", CELL_NAMES)
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_cell_launch_bits_fp64_and_virial(dev, mid, cname, case):
    from colvarsfinder import _hip, export
    w = world(dev, mid, cname)
    s, X_all, layout, cols, xw = w["s"], w["X_all"], w["layout"], w["cols"], w["xw"]
    terms, (u_tol, du_tol, f_tol) = terms_of(s, case)
    desc, table = export.bias_desc(terms, s["k"], dev)
    # the launch that exists today, on the dense whole frames
    F_d = torch.zeros_like(xw)
    rc, xi_d, U_d, dU_d = T1.bias_call(s, desc, xw, F_d, Bc.B)
    assert rc == 0
    # the cell launch on the torn frames in the engine's arrays
    F_all = w["F_all"].clone()
    before = F_all.clone()
    vir = torch.full((Bc.B, 9), NAN, device=dev)
    mc = _hip.MDCell(w["cell_t"].data_ptr(), w["stride"], vir.data_ptr())
    rc, xi, U, dU = cell_call(s, desc, X_all, F_all, Bc.B, layout, mc)
    assert rc == 0, _hip.lib().cvf_last_error().decode()
    assert torch.equal(xi, xi_d) and torch.equal(U, U_d) and torch.equal(dU, dU_d)
    touched = torch.zeros_like(F_all, dtype=torch.bool)
    touched[:, cols] = True
    assert torch.equal(F_all[:, cols], before[:, cols] + F_d)                        # fp32(before + the namesake's force)
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32))
    assert (F_d != 0).any() and not torch.isnan(vir).any()
    # without the virial, and without du_rows: the same bits
    F2 = before.clone()
    rc, xi2, U2, _ = cell_call(s, desc, X_all, F2, Bc.B, layout, _hip.MDCell(w["cell_t"].data_ptr(), w["stride"], None), want_du=False)
    assert rc == 0 and torch.equal(F2, F_all) and torch.equal(xi2, xi) and torch.equal(U2, U)
    # a second call adds the same again
    once = F_all.clone()
    vir2 = torch.full((Bc.B, 9), NAN, device=dev)
    rc, _, _, _ = cell_call(s, desc, X_all, F_all, Bc.B, layout, _hip.MDCell(w["cell_t"].data_ptr(), w["stride"], vir2.data_ptr()))
    assert rc == 0 and torch.equal(F_all[:, cols], once[:, cols] + F_d) and torch.equal(vir2, vir)
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32))
    # frame b alone gives its batch bits, the virial's too
    for b in range(Bc.B):
        F1 = before[b:b + 1].clone()
        v1 = torch.full((1, 9), NAN, device=dev)
        cb = w["cell_t"][b] if w["stride"] else w["cell_t"]
        rc, xi1, U1, dU1 = cell_call(s, desc, X_all[b:b + 1].contiguous(), F1, 1, layout, _hip.MDCell(cb.data_ptr(), 0, v1.data_ptr()))
        assert rc == 0 and torch.equal(xi1[0], xi[b]) and torch.equal(U1[0], U[b]) and torch.equal(dU1[0], dU[b])
        assert torch.equal(F1[0], once[b]) and torch.equal(v1[0], vir[b]), b
    # ---- against fp64: the sequential rule in numpy, then autograd of U(xi(.)) and of U(xi((I + eps) .))
    shape = np.asarray(s["frames"]).shape
    U64, dU64, F64 = B2.reference(mid, s["nets"], w["w64"].reshape(shape), terms)
    eu, ed, ef = Bc.rel_rows(U.cpu().numpy(), U64), Bc.rel_rows(dU.cpu().numpy(), dU64), Bc.rel_rows(F_d.cpu().numpy(), F64)
    R = torch.tensor(w["w64"])                                                       # [B, n, 3]
    eps = torch.zeros(Bc.B, 3, 3, dtype=torch.float64, requires_grad=True)
    Xs = torch.einsum("bij,baj->bai", torch.eye(3, dtype=torch.float64) + eps, R).reshape(shape)
    B2.ref_bias2(terms, Bc.xi_of(mid, s["nets"], Xs, torch.float64)).sum().backward()
    V64 = -eps.grad.transpose(1, 2).numpy().reshape(Bc.B, 9)                         # sum_a r_a (x) f_a
    scale = (np.linalg.norm(w["w64"], axis=2) * np.linalg.norm(F64.reshape(Bc.B, -1, 3), axis=2)).sum(axis=1)     # [B]
    ev = float((np.abs(vir.cpu().numpy().astype(np.float64) - V64).max(axis=1) / scale).max())
    plain = torch.einsum("bai,baj->bij", xw.view(Bc.B, -1, 3), F_d.view(Bc.B, -1, 3)).reshape(Bc.B, 9)           # torch fp32, the launch's own outputs
    ep = float((np.abs(plain.cpu().numpy().astype(np.float64) - V64).max(axis=1) / scale).max())
    print(f"[cvcell] {mid} {cname} {case}: U {eu:.2e} dU {ed:.2e} force {ef:.2e} virial {ev:.2e} (torch fp32 of the outputs {ep:.2e})")
    assert np.isfinite(F64).all() and np.abs(F64).max() > 1e-3 and (scale > 0).all()
    assert eu <= u_tol and ed <= du_tol and ef <= f_tol
    assert ev <= V_TOL


@pytest.mark.parametrize("mid", ALL_MODELS)
def test_cell_launch_bits_on_a_cell_whose_shifts_round(dev, mid):
    """The host test's triclinic cell (nothing exact in fp32): every kernel instance subtracts the shift as cvf_md_make_whole and the host
    program do, to the last bit - xi_rows, u_rows, du_rows, the force and the virial's inputs."""
    from colvarsfinder import _hip, export
    w = world(dev, mid, "triclinic")
    s, xw, cols = w["s"], w["xw"], w["cols"]
    terms, _ = terms_of(s, "harmonic")
    desc, table = export.bias_desc(terms, s["k"], dev)
    F_d = torch.zeros_like(xw)
    rc, xi_d, U_d, dU_d = T1.bias_call(s, desc, xw, F_d, Bc.B)
    assert rc == 0
    F_all = w["F_all"].clone()
    before = F_all.clone()
    vir = torch.full((Bc.B, 9), NAN, device=dev)
    rc, xi, U, dU = cell_call(s, desc, w["X_all"], F_all, Bc.B, w["layout"], _hip.MDCell(w["cell_t"].data_ptr(), 0, vir.data_ptr()))
    assert rc == 0, _hip.lib().cvf_last_error().decode()
    assert torch.equal(xi, xi_d) and torch.equal(U, U_d) and torch.equal(dU, dU_d) and (F_d != 0).any()
    assert torch.equal(F_all[:, cols], before[:, cols] + F_d)
    touched = torch.zeros_like(F_all, dtype=torch.bool)
    touched[:, cols] = True
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32)) and not torch.isnan(vir).any()


@pytest.mark.parametrize("mid", ["wave-A", "wave-identity", "large-C", "large-A-weighted"])
def test_virial_without_a_cell_keeps_the_layout_launchs_bits(dev, mid):
    from colvarsfinder import _hip, export
    s = T1.setup(dev, mid)
    terms, _ = terms_of(s, "harmonic")
    desc, table = export.bias_desc(terms, s["k"], dev)
    X_all, F_all, layout, index, cols = engine_arrays(s["x"], dev, seed=5)
    Fp = F_all.clone()
    rc, xi_p, U_p, dU_p = T1.bias_call(s, desc, X_all, Fp, Bc.B, layout)
    assert rc == 0
    vir = torch.full((Bc.B, 9), NAN, device=dev)
    Fc = F_all.clone()
    rc, xi, U, dU = cell_call(s, desc, X_all, Fc, Bc.B, layout, _hip.MDCell(None, 0, vir.data_ptr()))
    assert rc == 0 and torch.equal(Fc.view(torch.int32), Fp.view(torch.int32)) and torch.equal(xi, xi_p) and torch.equal(U, U_p) and torch.equal(dU, dU_p)
    force = (Fc - F_all)[:, cols]
    want = torch.einsum("bai,baj->bij", s["x"].double().view(Bc.B, -1, 3), (Fc[:, cols].double() - F_all[:, cols].double()).view(Bc.B, -1, 3))
    assert not torch.isnan(vir).any() and (force != 0).any()
    assert float((vir.double().view(Bc.B, 3, 3) - want).abs().max() / want.abs().max()) < 1e-4      # (the added force is seen through F's rounding)


def test_refusals_leave_everything_untouched(dev):
    from colvarsfinder import _hip, export
    from colvarsfinder.pp import identity_desc
    from tests import cv_frame_cases as Fc
    lib = _hip.lib()
    for mid in ("wave-A", "large-C"):
        w = world(dev, mid, "ortho")
        s = w["s"]
        terms, _ = terms_of(s, "harmonic")
        desc, table = export.bias_desc(terms, s["k"], dev)
        F_all = w["F_all"].clone()
        before = F_all.clone()
        vir = torch.full((Bc.B, 9), 3.25, device=dev)
        cp, vp = w["cell_t"].data_ptr(), vir.data_ptr()
        for name, mc, words in (("negative stride", _hip.MDCell(cp, -9, vp), "cell_frame_stride = -9"), ("nothing asked", _hip.MDCell(None, 0, None), "both NULL"),
                                ("no struct", None, "cell is NULL")):
            rc, xi, U, dU = cell_call(s, desc, w["X_all"], F_all, Bc.B, w["layout"], mc)
            why = lib.cvf_last_error().decode()
            assert rc < 0 and words in why, (name, rc, why)
            assert torch.isnan(xi).all() and torch.isnan(U).all() and torch.isnan(dU).all() and (vir == 3.25).all(), name
            assert torch.equal(F_all.view(torch.int32), before.view(torch.int32)), name
        # what the namesake refuses is refused here too
        bad = _hip.BiasDesc.from_buffer_copy(desc)
        bad.term[0].cv = s["k"]
        rc, xi, U, dU = cell_call(s, bad, w["X_all"], F_all, Bc.B, w["layout"], _hip.MDCell(cp, 0, vp))
        assert rc < 0 and "term[0].cv" in lib.cvf_last_error().decode() and torch.isnan(xi).all() and (vir == 3.25).all()
        assert torch.equal(F_all.view(torch.int32), before.view(torch.int32))
    # frames that are no whole atoms (CVF_PP_IDENTITY, n_coord = 4)
    m, pdesc, theta = Fc.mlp([4, 5, 1], 2), identity_desc(4), torch.zeros(64, device=dev)
    assert lib.cvf_cv_frame_bias_supported(m, 2, pdesc) == 1 and lib.cvf_cv_frame_bias_cell_supported(m, 2, pdesc) == 0
    assert "n_coord = 4" in lib.cvf_last_error().decode()
    x4, f4, xi, U = torch.zeros(1, 8, device=dev), torch.full((1, 8), 2.0, device=dev), torch.full((1, 2), NAN, device=dev), torch.full((1,), NAN, device=dev)
    vir, cell = torch.full((1, 9), 3.25, device=dev), torch.tensor(Cc.ORTHO, dtype=torch.float32, device=dev)
    rc = lib.cvf_cv_frame_bias_cell_eval(m, _hip.ptr(theta), 2, pdesc, _hip.BiasDesc(), None, _hip.ptr(x4), 1, _hip.ptr(xi), _hip.ptr(U), None,
                                         _hip.ptr(f4), _hip.stream(), _hip.MDCell(cell.data_ptr(), 0, vir.data_ptr()))
    torch.cuda.synchronize()
    why = lib.cvf_last_error().decode()
    assert rc < 0 and "n_coord = 4" in why and "CVF_PP_IDENTITY" in why, why
    assert torch.isnan(xi).all() and torch.isnan(U).all() and (f4 == 2.0).all() and (vir == 3.25).all()


def boundary_layer(n_atoms, dev):
    from colvarsfinder import pp
    rs = np.random.RandomState(1)
    ref = rs.normal(size=(n_atoms, 3))
    align = [0, 1, 2, 3]
    return pp.AlignFeatureLayer(n_atoms, align, ref[align], [("bond", (0, n_atoms - 1)), ("angle", (1, 2, 3))], False).to(dev), ref


def test_cell_supported_counts_four_bytes_per_atom(dev):
    """No entry of the case tables fills the LDS with its image counts, so one is built at the boundary: a CV over a frame of 40 950
    atoms (four aligned, two features).  The namesake takes it; with 4 bytes per atom more it is past 160 KiB and declined by name,
    and the last size that fits is exactly the one the limit 160 KiB - 4 n_atoms gives."""
    from colvarsfinder import _hip, core, export, nn
    lib = _hip.lib()
    n_atoms = 40950
    layer, ref = boundary_layer(n_atoms, dev)
    torch.manual_seed(3)
    nets = nn.EigenFunctions([layer.d_r, 5, 1], 2, activation=torch.nn.Tanh())
    mdesc, cut, k, theta, ns = Bc.plan_of(nets)
    pdesc = layer.pp_desc()
    assert lib.cvf_cv_frame_large_bias_supported(mdesc, cut, pdesc) == 1
    assert lib.cvf_cv_frame_large_bias_cell_supported(mdesc, cut, pdesc) == 0
    why = lib.cvf_last_error().decode()
    assert "cvf_cv_frame_large_bias_cell" in why and "image counts" in why and str(4 * n_atoms) in why and "three-call" in why, why
    # the boundary: the one-row launch's own bytes plus 4 per atom against 160 KiB (the predicate reads only n_coord of a frame's size)
    small = _hip.PPDesc.from_buffer_copy(pdesc)
    small.n_coord = 3
    small_atoms = 1
    assert lib.cvf_cv_frame_large_bias_cell_supported(mdesc, cut, small) == 1
    lo, hi = small_atoms, n_atoms            # supported at lo, declined at hi
    while hi - lo > 1:
        mid_ = (lo + hi) // 2
        small.n_coord = 3 * mid_
        lo, hi = (mid_, hi) if lib.cvf_cv_frame_large_bias_cell_supported(mdesc, cut, small) == 1 else (lo, mid_)
    small.n_coord = 3 * hi
    assert lib.cvf_cv_frame_large_bias_cell_supported(mdesc, cut, small) == 0
    needed = int(lib.cvf_last_error().decode().split("needs ")[1].split(" bytes")[0])
    assert needed == 160 * 1024 + 4 and needed - 4 * hi + 4 * lo == 160 * 1024          # one atom past the limit; lo fills it exactly
    # BiasedCV reports the routes: the namesake's launch without a cell, the three calls with one
    cv = core._CVModel(layer, nets.to(dev), device=dev)
    bc = export.BiasedCV(cv, [("harmonic", 0, 1.0, 0.0)], dev, large_frames=True)
    assert bc.route == "frame-large" and bc.route_cell == "three-call" and "image counts" in bc.supported_large_cell[1]


# ------------------------------------------------------------------------------------------------ export.BiasedCV, export.make_whole
def ref_of(terms, nets, torch_layer64, w64):
    import copy
    X = torch.tensor(w64, dtype=torch.float64, requires_grad=True)
    xi64 = copy.deepcopy(nets).to("cpu", torch.float64)(torch_layer64(X)).reshape(X.shape[0], -1)
    U64 = Bc.ref_bias(terms, xi64)
    U64.sum().backward()
    return U64.detach().numpy(), -X.grad.reshape(X.shape[0], -1).numpy()


def test_biased_cv_routes_on_torn_input(dev):
    """("mixed65", "A-k3") of tests/cv_frame_large_cases: the three calls (behind cvf_md_make_whole) and the workgroup launch, and
    wave-A on the wave launch - each on torn frames against fp64, the first two against each other; cell=None gives today's bits."""
    import copy
    from colvarsfinder import core, export
    from tests import cv_frame_large_cases as G
    layer, nets = G.hip_layer("mixed65", dev), G.nets_for("mixed65", "A-k3")
    traj, _ = G.frames("mixed65")
    cv = core._CVModel(layer, copy.deepcopy(nets).to(dev), device=dev)
    x = torch.tensor(traj, device=dev).reshape(Bc.B, -1).contiguous()
    xi0, _ = export.FrameCV(cv, dev)(x)
    terms = Bc.terms_for("three-on-one", xi0.cpu().numpy()) + [{"kind": "harmonic", "cv": 2, "kappa": 0.9, "center": float(xi0[:, 2].min() - 1.5)}]
    cells = scaled_cells(traj, "per-frame")
    torn = torn_frames(traj, cells, G.parts("mixed65")[1], seed=65)
    w64 = np.stack([Cc.whole_fp64(cells[b], torn[b])[0] for b in range(Bc.B)])
    U64, F64 = ref_of(terms, nets, G.torch_layer("mixed65", torch.float64), w64)
    xt = torch.tensor(torn.reshape(Bc.B, -1), device=dev)
    cell_t = torch.tensor(cells, device=dev)
    three, large = export.BiasedCV(cv, terms, dev), export.BiasedCV(cv, terms, dev, large_frames=True)
    assert three.route_cell == "three-call" and large.route_cell == "frame-large"
    xw = export.make_whole(xt.view(Bc.B, -1, 3), cell_t)
    assert xw.shape == (Bc.B, 65, 3) and np.abs(xw.cpu().numpy() - w64).max() <= 2 * Cc.EPS * np.abs(w64).max()
    out = {}
    for name, bc in (("three-call", three), ("frame-large", large)):
        F, V = torch.zeros_like(xt), torch.full((Bc.B, 3, 3), NAN, device=dev)
        _, U, _ = bc(xt, F, cell=cell_t, virial=V)
        out[name] = (U.cpu().numpy(), F.cpu().numpy(), V.cpu().numpy())
        eu, ef = Bc.rel_rows(out[name][0], U64), Bc.rel_rows(out[name][1], F64)
        print(f"[cvcell] BiasedCV mixed65 A-k3 {name} torn: U {eu:.2e} force {ef:.2e}")
        assert eu <= Bc.U_TOL and ef <= Bc.F_TOL
        # cell=None: today's call on the whole frames, bit for bit the call without the keyword
        Fa, Fb = torch.zeros_like(xt), torch.zeros_like(xt)
        ra, rb = bc(xw.view(Bc.B, -1), Fa), bc(xw.view(Bc.B, -1), Fb, cell=None, virial=None)
        assert torch.equal(Fa, Fb) and all(torch.equal(p, q) for p, q in zip(ra, rb))
    d_u, d_f = Bc.rel_rows(out["three-call"][0], out["frame-large"][0]), Bc.rel_rows(out["three-call"][1], out["frame-large"][1])
    d_v = float(np.abs(out["three-call"][2] - out["frame-large"][2]).max() / np.abs(out["frame-large"][2]).max())
    print(f"[cvcell] BiasedCV mixed65 A-k3 three-call against frame-large, torn: U {d_u:.2e} force {d_f:.2e} virial {d_v:.2e}")
    assert d_u <= Bc.U_TOL and d_f <= Bc.F_TOL and d_v <= V_ROUTE_TOL
    # the wave launch, through the engine's layout
    w = world(dev, "wave-A", "dyadic")
    s, cvw = T1.cv_model("wave-A", dev)
    termsw, (u_tol, du_tol, f_tol) = terms_of(s, "harmonic")
    bw = export.BiasedCV(cvw, termsw, dev, atom_index=w["index"].cpu(), atom_stride=4)
    assert bw.route_cell == "frame"
    F = torch.zeros_like(w["F_all"])
    _, U, _ = bw(w["X_all"], F, cell=w["cell_t"])
    U64, _, F64 = Bc.reference("wave-A", s["nets"], w["w64"], termsw)
    eu, ef = Bc.rel_rows(U.cpu().numpy(), U64), Bc.rel_rows(F[:, w["cols"]].cpu().numpy(), F64)
    print(f"[cvcell] BiasedCV wave-A frame torn: U {eu:.2e} force {ef:.2e}")
    assert eu <= u_tol and ef <= f_tol


def test_a_captured_call_follows_the_cell(dev):
    """The cell is read at launch time: a call captured in a graph, then the cell and the wrapped positions rescaled in place by 1.01
    (a barostat step) and the graph replayed - the bits of the eager call on the rescaled arrays."""
    from colvarsfinder import export
    w = world(dev, "wave-A", "dyadic")
    s, cv = T1.cv_model("wave-A", dev)
    terms, _ = terms_of(s, "harmonic")
    bc = export.BiasedCV(cv, terms, dev, atom_index=w["index"].cpu(), atom_stride=4)
    X, cell = w["X_all"].clone(), w["cell_t"].clone()
    F, V = torch.zeros_like(w["F_all"]), torch.zeros(Bc.B, 9, device=dev)
    bc(X, F, cell=cell, virial=V)            # (warm-up: attributes, allocator)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    F.zero_()
    with torch.cuda.graph(graph):
        xi, U, dU = bc(X, F, cell=cell, virial=V)
    graph.replay()
    torch.cuda.synchronize()
    first = (xi.clone(), U.clone(), F.clone(), V.clone())
    cell.mul_(1.01)
    X.mul_(1.01)
    F.zero_()
    graph.replay()
    torch.cuda.synchronize()
    F2, V2 = torch.zeros_like(F), torch.zeros_like(V)
    xi2, U2, dU2 = bc(X, F2, cell=cell, virial=V2)
    torch.cuda.synchronize()
    assert torch.equal(xi, xi2) and torch.equal(U, U2) and torch.equal(dU, dU2) and torch.equal(F, F2) and torch.equal(V, V2)
    assert not torch.equal(first[0], xi) and (F != 0).any()
