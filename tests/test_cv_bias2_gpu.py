"""GPU (-m gpu): joint 2-D grid bias terms inside the one-launch bias kernels (csrc/cv_bias.hip), hill deposition on the device
(cvf_cv_bias_deposit, csrc/cv_bias_hills.hip) and export.BiasedCV.deposit; DESIGN.md section 4.19.  Grids, hills, the independent
fp64 reference, the host program and the bars: tests/cv_bias2_cases.py; models, frames and launch helpers: tests/cv_bias_cases.py and
tests/test_cv_bias_gpu.py (whose per-model setup is built once and shared).  B = 3 frames on the eight bias models.

  bits     xi_rows and the force added to a zero-filled dense F_all are the namesake's coef form with coef = -du_rows (torch.equal)
  fp64     U, dU and the force against torch fp64 autograd of U(xi(x)), the bias written independently
  deposit  table and hills against fp64 and against the host program tools/bias2_host.cpp; geometry, chunking, refusals, a captured
           step.  The program is built here WITHOUT sanitizers (a plain host executable): the CPU tests run it under the address and
           undefined-behaviour sanitizers and check that both builds print the same bits; no sanitizer runs in this module"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cv_bias2_cases as B2
from tests import cv_bias_cases as Bc
from tests import test_cv_bias_gpu as T1

pytestmark = pytest.mark.gpu
NAN = float("nan")
ALL_MODELS = Bc.MODELS_WAVE + Bc.MODELS_LARGE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return B2.build_program(tmp_path_factory.mktemp("bias2"), sanitize=False)


def grid_of(s, case, dev):
    from colvarsfinder import export
    terms = B2.grid_terms(case, s["xi0"].cpu().numpy())
    desc, table = export.bias_desc(terms, s["k"], dev)
    return terms, desc, table


# ------------------------------------------------------------------------------------------------ the 2-D term in the one launch
@pytest.mark.parametrize("case", B2.GRID_CASES)
@pytest.mark.parametrize("mid", ALL_MODELS)
def test_grid_term_bits_and_fp64(dev, mid, case):
    s = T1.setup(dev, mid)
    terms, desc, table = grid_of(s, case, dev)
    xi, U, dU, F = T1.dense(s, desc)
    assert not torch.isnan(xi).any() and not torch.isnan(U).any() and not torch.isnan(dU).any() and not torch.isnan(F).any()
    # bits: the namesake's xi and its coef form
    assert torch.equal(xi, s["xi0"])
    _, Fn = T1.namesake(s, s["x"], coef=(-dU).contiguous())
    assert torch.equal(F, Fn) and (dU != 0).any() and (F != 0).any()
    # a second call adds the same again; a frame alone gives the bits it has in the batch
    F2 = F.clone()
    rc, _, U2, dU2 = T1.bias_call(s, desc, s["x"], F2, Bc.B)
    assert rc == 0 and torch.equal(F2, F + F) and torch.equal(U2, U) and torch.equal(dU2, dU)
    for b in range(Bc.B):
        F1 = torch.zeros_like(F[b:b + 1])
        rc, xi1, U1, dU1 = T1.bias_call(s, desc, s["x"][b:b + 1].contiguous(), F1, 1)
        assert rc == 0 and torch.equal(xi1[0], xi[b]) and torch.equal(U1[0], U[b]) and torch.equal(dU1[0], dU[b]) and torch.equal(F1[0], F[b])
    # fp64: the bias written independently, autograd through the oracle's layer and the nets
    U64, dU64, F64 = B2.reference(mid, s["nets"], s["frames"], terms)
    eu, ed, ef = Bc.rel_rows(U.cpu().numpy(), U64), Bc.rel_rows(dU.cpu().numpy(), dU64), Bc.rel_rows(F.cpu().numpy(), F64)
    print(f"[cvbias2] {mid} {case}: U {eu:.2e} dU {ed:.2e} force {ef:.2e}")
    # frame 0 lies where the case says, by the reference's xi (a change of model cannot silently drop the coverage)
    X = torch.tensor(np.asarray(s["frames"]), dtype=torch.float64)
    xi64 = Bc.xi_of(mid, s["nets"], X, torch.float64).detach().numpy()
    where, cell = B2.region(terms[0], xi64[0])
    assert where == B2.REGION_OF[case], (case, where, cell)
    if case == "on-node":       # exactly on node (2, 1), in the fp32 arithmetic of the kernel
        t = terms[0]
        lo, inv_h = B2.term_axes(t)
        x0 = s["xi0"][0].cpu().numpy()
        assert (np.float32(x0[t["cv"]]) - np.float32(lo[0])) * np.float32(inv_h[0]) == 2.0
        assert (np.float32(x0[t["cv2"]]) - np.float32(lo[1])) * np.float32(inv_h[1]) == 1.0
        node = B2.term_nodes(t)[2, 1].astype(np.float32)
        assert U[0].item() == node[0] and dU[0, t["cv"]].item() == node[1] and dU[0, t["cv2"]].item() == node[2]
    if case == "cv-swapped":
        assert terms[0]["cv"] > terms[0]["cv2"]
    assert np.isfinite(F64).all() and np.abs(F64).max() > 1e-3
    assert eu <= B2.U_TOL and ed <= B2.DU_TOL and ef <= B2.F_TOL


@pytest.mark.parametrize("mid", ["wave-A", "large-A-weighted"])
def test_engine_layout(dev, mid):
    """A shuffled atom index over atoms of 4 floats: X_all is NaN wherever it must not be read, F_all random wherever it must not be
    written; the untouched bits are kept."""
    s = T1.setup(dev, mid)
    _, desc, table = grid_of(s, "plus-harmonic", dev)
    xi_d, U_d, dU_d, F_d = T1.dense(s, desc)
    X_all, F_all, layout, index, cols = T1.engine_arrays(s, dev, seed=5 + len(mid))
    before = F_all.clone()
    rc, xi, U, dU = T1.bias_call(s, desc, X_all, F_all, Bc.B, layout)
    assert rc == 0 and torch.equal(xi, xi_d) and torch.equal(U, U_d) and torch.equal(dU, dU_d)
    touched = torch.zeros_like(F_all, dtype=torch.bool)
    touched[:, cols] = True
    assert torch.equal(F_all[~touched].view(torch.int32), before[~touched].view(torch.int32))
    assert torch.equal(F_all[:, cols], before[:, cols] + F_d) and (F_d != 0).any()


# ------------------------------------------------------------------------------------------------ deposit through the C ABI
def deposit(desc, k, hill, xi_rows, table, hills, table_arg=None, B=None):
    from colvarsfinder import _hip
    rc = _hip.lib().cvf_cv_bias_deposit(desc, k, hill, _hip.ptr(xi_rows), xi_rows.shape[0] if B is None else B,
                                        _hip.ptr(table) if table_arg is None else table_arg, _hip.ptr(hills), _hip.stream())
    torch.cuda.synchronize()
    return rc


def hill_desc(term, height, sigma, sigma2, inv_kdt):
    from colvarsfinder import _hip
    return _hip.HillDesc(term, 0, height, sigma, sigma2, inv_kdt)


@pytest.mark.parametrize("inv_kdt", [0.0, 0.8], ids=["plain", "well-tempered"])
@pytest.mark.parametrize("dim", [1, 2])
def test_deposit_matches_fp64_and_the_host_program(dev, program, dim, inv_kdt):
    """The host test's cases - three hills (inside, outside, a NaN centre) onto smooth nodes, twice - against the same fp64 reference
    and against the table of the host program (its plain build; the CPU tests tie it to the sanitized one); two runs from the same table give the same bits."""
    from colvarsfinder import export
    term = B2.deposit_terms(dim, True)
    k, centres = (1, B2.HILLS_1D) if dim == 1 else (2, B2.HILLS_2D)
    sigma = (0.3, 0.0) if dim == 1 else (0.3, 0.55)
    desc, table = export.bias_desc([term], k, dev)
    table0 = table.clone()
    xi_rows = torch.tensor(centres, device=dev)
    hill = hill_desc(0, 1.2, sigma[0], sigma[1], inv_kdt)
    got = []
    for run in range(2):
        table.copy_(table0)
        hills = [torch.full((3, 4), NAN, device=dev) for _ in range(2)]
        for h in hills:
            assert deposit(desc, k, hill, xi_rows, table, h) == 0
        got.append((table.clone(), torch.cat(hills)))
    assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32))
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    T, H = got[0][0].cpu().numpy().astype(np.float64), got[0][1].cpu().numpy().astype(np.float64)
    nodes0 = B2.nodes_of(term)
    sig = sigma[0] if dim == 1 else sigma
    nodes1, hills1 = B2.ref_deposit(term, nodes0, np.float32(centres), 1.2, sig, inv_kdt)
    nodes2, hills2 = B2.ref_deposit(term, nodes1, np.float32(centres), 1.2, sig, inv_kdt)
    for g, want in ((H[:3], hills1), (H[3:], hills2)):
        assert g[2, 2] == 0.0 and np.isnan(g[2, 0]) and np.array_equal(g[:2, :2], want[:2, :2])
        eh = np.abs(g[:2, 2:] - want[:2, 2:]).max() / np.abs(want[:2, 2:]).max()
        print(f"[cvbias2] deposit {dim}-D inv_kdt {inv_kdt}: heights against fp64 {eh / B2.EPS:.2f} eps")
        assert eh <= B2.DEP_GPU_TOL
    err = B2.rel_cols(T.reshape(nodes2.shape), nodes2)
    call = (0, 1.2, sigma[0], sigma[1], inv_kdt, centres)
    _, Hh, Th = program([term], k, deposits=[call, call])
    err_host = B2.rel_cols(T.reshape(nodes2.shape), Th.reshape(nodes2.shape))
    print(f"[cvbias2] deposit {dim}-D inv_kdt {inv_kdt}: table against fp64 {err / B2.EPS:.2f} eps, against the host program {err_host / B2.EPS:.2f} eps")
    assert err <= B2.DEP_GPU_TOL and err_host <= B2.DEP_GPU_TOL
    assert np.abs(H[:, 2] - Hh[:, 2]).max() <= B2.DEP_GPU_TOL * 1.2


@pytest.mark.parametrize("dim", [1, 2])
def test_one_call_of_three_hills_is_three_calls_of_one(dev, dim):
    """inv_kdt = 0: no height depends on the table, and a node adds its hills in the order b = 0 .. B - 1 either way."""
    from colvarsfinder import export
    term = B2.deposit_terms(dim, True)
    k = dim
    centres = [[0.07], [1.3], [-0.4]] if dim == 1 else [[0.07, 0.9], [0.8, 2.2], [-0.3, 0.4]]
    desc, table = export.bias_desc([term], k, dev)
    table0 = table.clone()
    xi_rows = torch.tensor(centres, device=dev)
    hill = hill_desc(0, 0.9, 0.3, 0.55, 0.0)
    hills = torch.full((3, 4), NAN, device=dev)
    assert deposit(desc, k, hill, xi_rows, table, hills) == 0
    once = table.clone()
    table.copy_(table0)
    rows = torch.full((3, 4), NAN, device=dev)
    for b in range(3):
        assert deposit(desc, k, hill, xi_rows[b:b + 1].contiguous(), table, rows[b:b + 1]) == 0
    assert torch.equal(table.view(torch.int32), once.view(torch.int32)) and not torch.equal(once, table0)
    assert torch.equal(rows[:, :3], hills[:, :3]) and (hills[:, 2] == 0.9).all()         # (V_b is the table's before each call: it differs)


def test_more_than_one_workgroup_and_more_than_one_chunk(dev):
    """33 x 9 = 297 nodes - more than one workgroup of 256 and no multiple of it - and B = CVF_HILL_CHUNK + 1 hills, behind a 1-D term
    of 3 nodes (6 floats: the grid starts at float 8): against fp64, and bit for bit against B calls of one hill."""
    from colvarsfinder import _hip, export
    n1, n2, B = 33, 9, _hip.HILL_CHUNK + 1
    grid = {"kind": "table2d", "cv": 1, "cv2": 0, "lo": (-1.0, -0.5), "h": (0.0625, 0.125), "n": (n1, n2)}
    first = {"kind": "table", "cv": 0, "lo": 0.0, "h": 0.5, "u": [1.0, 2.0, 3.0], "du": [0.5, 0.25, 0.125]}
    desc, table = export.bias_desc([first, grid], 2, dev)
    assert desc.term[1].tab_off == 8 and desc.n_table == 8 + 4 * n1 * n2
    rs = np.random.RandomState(11)
    centres = np.stack([rs.uniform(-0.7, 0.7, B), rs.uniform(-1.2, 1.2, B)], axis=1).astype(np.float32)      # (xi_0 = cv2, xi_1 = cv)
    xi_rows = torch.tensor(centres, device=dev)
    hill = hill_desc(1, 0.05, 0.2, 0.15, 0.0)
    hills = torch.full((B, 4), NAN, device=dev)
    assert deposit(desc, 2, hill, xi_rows, table, hills) == 0
    got = table.cpu().numpy()
    assert np.array_equal(got[:8], np.float32([1.0, 0.5, 2.0, 0.25, 3.0, 0.125, 0.0, 0.0]))                   # the neighbours' bits
    ref_term = dict(grid, inv_h=(16.0, 8.0), **{key: np.zeros((n1, n2)) for key in ("u", "d1", "d2", "d12")})
    nodes, hills64 = B2.ref_deposit(ref_term, np.zeros((n1, n2, 4)), centres[:, [1, 0]], 0.05, (0.2, 0.15), 0.0)
    err = B2.rel_cols(got[8:].reshape(n1, n2, 4), nodes)
    print(f"[cvbias2] deposit 33 x 9, {B} hills: table against fp64 {err / B2.EPS:.2f} eps")
    assert err <= B2.DEP_GPU_TOL
    assert np.array_equal(hills.cpu().numpy()[:, :2], centres[:, [1, 0]]) and (hills[:, 2] == float(np.float32(0.05))).all() and (hills[:, 3] == 0).all()
    once = table.clone()
    table[8:] = 0.0
    row = torch.full((1, 4), NAN, device=dev)
    for b in range(B):
        assert deposit(desc, 2, hill, xi_rows[b:b + 1].contiguous(), table, row) == 0
    assert torch.equal(table.view(torch.int32), once.view(torch.int32))


def test_deposit_refusals_leave_table_and_hills_untouched(dev):
    from colvarsfinder import _hip, export
    lib = _hip.lib()
    terms = [{"kind": "harmonic", "cv": 0, "kappa": 1.0, "center": 0.0}, B2.deposit_terms(2, True), dict(B2.deposit_terms(1, True), cv=1)]
    desc, table = export.bias_desc(terms, 2, dev)
    table.copy_(torch.arange(table.numel(), device=dev) * 0.25 + 7.0)
    before = table.clone()
    xi_rows = torch.tensor(B2.HILLS_2D, device=dev)
    hills = torch.full((3, 4), -5.5, device=dev)
    INF = float("inf")
    good = lambda: hill_desc(1, 1.2, 0.3, 0.55, 0.8)

    def changed(**fields):
        h = good()
        for name, value in fields.items():
            setattr(h, name, value)
        return h

    bad_desc = _hip.BiasDesc.from_buffer_copy(desc)
    bad_desc.term[1].cv2 = 0
    other = torch.zeros_like(table)
    cases = [("the bias check", dict(d=bad_desc), "term[1].cv2"), ("term == n_terms", dict(h=changed(term=3)), "hill.term = 3"),
             ("negative term", dict(h=changed(term=-1)), "hill.term = -1"), ("no table term", dict(h=changed(term=0)), "hill.term = 0"),
             ("height 0", dict(h=changed(height=0.0)), "hill.height"), ("negative height", dict(h=changed(height=-1.0)), "hill.height"),
             ("NaN height", dict(h=changed(height=NAN)), "hill.height"), ("infinite height", dict(h=changed(height=INF)), "hill.height"),
             ("sigma 0", dict(h=changed(sigma=0.0)), "hill.sigma"), ("tiny sigma", dict(h=changed(sigma=1e-20)), "1 / sigma^2"), ("NaN sigma", dict(h=changed(sigma=NAN)), "hill.sigma"),
             ("sigma2 0 in 2-D", dict(h=changed(sigma2=0.0)), "hill.sigma2"), ("infinite sigma2 in 2-D", dict(h=changed(sigma2=INF)), "hill.sigma2"),
             ("negative inv_kdt", dict(h=changed(inv_kdt=-0.5)), "hill.inv_kdt"), ("NaN inv_kdt", dict(h=changed(inv_kdt=NAN)), "hill.inv_kdt"),
             ("another table", dict(table_arg=_hip.ptr(other)), "bias->table"), ("NULL table", dict(table_arg=C.c_void_p(None)), "table"),
             ("NULL xi_rows", dict(xi=None), "null"), ("NULL hills", dict(hills=None), "null"), ("NULL hill", dict(h=None), "hill"),
             ("NULL bias", dict(d=None), "bias"), ("B < 0", dict(B=-1), "B = -1")]
    for name, kw, word in cases:
        rc = lib.cvf_cv_bias_deposit(kw.get("d", desc), 2, kw.get("h", good()), _hip.ptr(kw.get("xi", xi_rows)), kw.get("B", 3),
                                     kw.get("table_arg", _hip.ptr(table)), _hip.ptr(kw.get("hills", hills)), _hip.stream())
        torch.cuda.synchronize()
        why = lib.cvf_last_error().decode()
        assert rc < 0 and word in why and why.startswith("cvf_cv_bias_deposit"), (name, rc, why)
        assert torch.equal(table.view(torch.int32), before.view(torch.int32)) and (hills == -5.5).all() and (other == 0).all(), name
    # sigma2 is not looked at for a 1-D term; B == 0 is a no-op
    h1 = hill_desc(2, 1.2, 0.3, -1.0, 0.0)
    assert lib.cvf_cv_bias_deposit(desc, 2, h1, _hip.ptr(xi_rows), 0, _hip.ptr(table), _hip.ptr(hills), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(table.view(torch.int32), before.view(torch.int32)) and (hills == -5.5).all()
    assert deposit(desc, 2, h1, xi_rows, table, hills) == 0
    d1 = desc.term[2]
    rest = torch.ones_like(table, dtype=torch.bool)
    rest[d1.tab_off:d1.tab_off + 2 * d1.n_nodes] = False
    assert torch.equal(table[rest].view(torch.int32), before[rest].view(torch.int32)) and not torch.equal(table[~rest], before[~rest])
    assert hills[2, 2].item() == np.float32(1.2) and hills[0, 1].item() == 0.0          # (the NaN is on CV 0: this term's centre is xi_1)


# ------------------------------------------------------------------------------------------------ export.BiasedCV.deposit
def empty_grid(xi0, k):
    """A zero-filled 5 x 4 grid on (CV 0, CV k - 1) with frame 0 inside cell (1, 1), as the "interior" case places it."""
    t = B2.grid_terms("interior", xi0)[0]
    return {"kind": "table2d", "cv": t["cv"], "cv2": t["cv2"], "lo": t["lo"], "inv_h": t["inv_h"], "n": (B2.N1, B2.N2)}


@pytest.mark.parametrize("mid,large,routes", [("wave-A", False, ("frame", "three-call")), ("large-A", True, ("frame-large", "three-call"))])
def test_biased_cv_deposit_on_every_route(dev, mid, large, routes):
    """A "table2d" term given by "n" starts at zero bias and zero force; bc.deposit at the current xi, then the next call: U, dU and
    the force match the fp64 reference "Hermite interpolation of the deposited nodes", and the routes agree within the bars.  The
    three-call route is taken on the same model by naming it (the route is the instance's attribute)."""
    from colvarsfinder import export
    s, cv = T1.cv_model(mid, dev)
    grid = empty_grid(s["xi0"].cpu().numpy(), s["k"])
    out = {}
    for route in routes:
        bc = export.BiasedCV(cv, [grid], dev, large_frames=large)
        assert bc.route == routes[0]
        bc.route = route
        F = torch.zeros_like(s["x"])
        xi, U, dU = bc(s["x"], F)
        assert (U == 0).all() and (dU == 0).all() and (F == 0).all() and (bc.table == 0).all()
        hills = bc.deposit(xi, 1.0, (0.3, 0.6), bias_factor=6.0, kT=0.5)
        assert hills.shape == (Bc.B, 4) and (hills[:, 2] == 1.0).all() and (hills[:, 3] == 0).all()      # (V = 0 everywhere: full heights)
        assert torch.equal(hills[:, 0], xi[:, grid["cv"]]) and torch.equal(hills[:, 1], xi[:, grid["cv2"]])
        hills2 = bc.deposit(xi, 1.0, (0.3, 0.6), term=0, bias_factor=6.0, kT=0.5)
        assert hills2[0, 2] < 1.0 and hills2[0, 3] > 0.5          # well-tempered: the bias is there now (frame 0 lies inside the grid)
        xi2, U, dU = bc(s["x"], F)
        assert torch.equal(xi2, xi)
        nodes = bc.table.cpu().numpy().astype(np.float64).reshape(B2.N1, B2.N2, 4)
        terms = [dict(grid, u=nodes[:, :, 0], d1=nodes[:, :, 1], d2=nodes[:, :, 2], d12=nodes[:, :, 3])]
        U64, dU64, F64 = B2.reference(mid, s["nets"], s["frames"], terms)
        out[route] = (U.cpu().numpy(), dU.cpu().numpy(), F.cpu().numpy())
        eu, ed, ef = Bc.rel_rows(out[route][0], U64), Bc.rel_rows(out[route][1], dU64), Bc.rel_rows(out[route][2], F64)
        print(f"[cvbias2] BiasedCV.deposit {mid} {route}: U {eu:.2e} dU {ed:.2e} force {ef:.2e}")
        assert U64[0] > 0.5 and eu <= B2.U_TOL and ed <= B2.DU_TOL and ef <= B2.F_TOL
        with pytest.raises(ValueError, match="go together"):
            bc.deposit(xi, 1.0, (0.3, 0.6), bias_factor=6.0)
        with pytest.raises(ValueError, match="hill.sigma2"):
            bc.deposit(xi, 1.0, 0.3)
    a, b = out[routes[0]], out[routes[1]]
    assert Bc.rel_rows(a[0], b[0]) <= B2.U_TOL and Bc.rel_rows(a[1], b[1]) <= B2.DU_TOL and Bc.rel_rows(a[2], b[2]) <= B2.F_TOL


def test_deposit_term_none_needs_exactly_one_table(dev):
    from colvarsfinder import export
    s, cv = T1.cv_model("wave-A", dev)
    grid = empty_grid(s["xi0"].cpu().numpy(), s["k"])
    two = export.BiasedCV(cv, [grid, {"kind": "table", "cv": 0, "lo": -1.0, "h": 0.5, "n": 6}], dev)
    none = export.BiasedCV(cv, [("harmonic", 0, 1.0, 0.0)], dev)
    for bc in (two, none):
        with pytest.raises(ValueError, match="exactly one table term"):
            bc.deposit(s["xi0"], 1.0, (0.3, 0.6))
    hills = two.deposit(s["xi0"], 0.7, 0.3, term=1)
    assert (hills[:, 2] == np.float32(0.7)).all() and (two.table[:80] == 0).all() and (two.table[80:] != 0).any()


# ------------------------------------------------------------------------------------------------ a captured step
@pytest.mark.parametrize("mid", ["wave-A", "large-C"])
def test_captured_eval_and_deposit_step(dev, mid):
    """One metadynamics step - the bias launch, then the deposit from the xi_rows it wrote - captured once on one stream and
    replayed three times: the table and U after each replay are the eager sequence's, bit for bit (well-tempered, so every step's
    heights depend on the step before)."""
    from colvarsfinder import _hip, export
    s = T1.setup(dev, mid)
    grid = empty_grid(s["xi0"].cpu().numpy(), s["k"])
    desc, table = export.bias_desc([grid], s["k"], dev)
    hill = hill_desc(0, 1.0, 0.3, 0.6, 1.0 / (5.0 * 0.5))
    k, P, lib = s["k"], _hip.ptr, _hip.lib()
    xi, U, dU = torch.zeros(Bc.B, k, device=dev), torch.zeros(Bc.B, device=dev), torch.zeros(Bc.B, k, device=dev)
    F, hills = torch.zeros_like(s["x"]), torch.zeros(Bc.B, 4, device=dev)

    def step():
        rc = s["bias"](s["mdesc"], P(s["theta"]), s["cut"], s["pdesc"], desc, None, P(s["x"]), Bc.B, P(xi), P(U), P(dU), P(F), _hip.stream())
        assert rc == 0, lib.cvf_last_error().decode()
        rc = lib.cvf_cv_bias_deposit(desc, k, hill, P(xi), Bc.B, P(table), P(hills), _hip.stream())
        assert rc == 0, lib.cvf_last_error().decode()

    eager = []
    for _ in range(3):
        step()
        torch.cuda.synchronize()
        eager.append((U.clone(), table.clone(), hills.clone()))
    assert (eager[0][0] == 0).all() and eager[1][0][0] > 0.5 and eager[2][0][0] > eager[1][0][0]      # (frame 0 lies inside the grid)
    table.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    assert (table == 0).all()            # capturing ran nothing
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((U, table, hills), eager[i]):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), i
