"""CPU: joint 2-D grid bias terms and hill deposition - the ABI, the description check, the Python
vocabulary, the deposit kernels' resources, and the formulas of csrc/cvf_bias.hpp compiled into the stand-alone host program
tools/bias2_host.cpp (with -fsanitize=address,undefined, a plain executable) against the fp64 definitions of
tests/cv_bias2_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import cv_bias2_cases as B2
from tests import cv_bias_cases as Bc

EPS = B2.EPS


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return B2.build_program(tmp_path_factory.mktemp("bias2"))


# ------------------------------------------------------------------------------------------------ ABI
def test_deposit_is_declared_bound_and_defined(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(hip.LIB_PATH)
    name = "cvf_cv_bias_deposit"
    assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name)
    assert set(hip._SIGNATURES) == declared


def test_struct_layouts_match_the_header(hip, tmp_path):
    """sizeof and the offset of every new field, as the C compiler lays the header's structs out."""
    cc = f"{codeobj.LLVM}/clang"
    assert os.path.exists(cc), f"{cc}: the toolchain that builds the library is missing"
    exprs = ["sizeof(cvf_bias_term)", "offsetof(cvf_bias_term, inv_h)", "offsetof(cvf_bias_term, cv2)", "offsetof(cvf_bias_term, n_nodes2)",
             "offsetof(cvf_bias_term, lo2)", "offsetof(cvf_bias_term, inv_h2)", "sizeof(cvf_bias_desc)", "offsetof(cvf_bias_desc, term)",
             "offsetof(cvf_bias_desc, table)", "sizeof(cvf_hill_desc)", "offsetof(cvf_hill_desc, term)", "offsetof(cvf_hill_desc, reserved)",
             "offsetof(cvf_hill_desc, height)", "offsetof(cvf_hill_desc, sigma)", "offsetof(cvf_hill_desc, sigma2)",
             "offsetof(cvf_hill_desc, inv_kdt)", "(size_t)CVF_HILL_CHUNK"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvf.h"\nint main(void) {\n'
                   + "".join(f'  printf("%zu\\n", {e});\n' for e in exprs) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I" + os.path.join(codeobj.ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.split()]
    T, D, H = hip.BiasTerm, hip.BiasDesc, hip.HillDesc
    want = [ctypes.sizeof(T), T.inv_h.offset, T.cv2.offset, T.n_nodes2.offset, T.lo2.offset, T.inv_h2.offset, ctypes.sizeof(D), D.term.offset,
            D.table.offset, ctypes.sizeof(H), H.term.offset, H.reserved.offset, H.height.offset, H.sigma.offset, H.sigma2.offset,
            H.inv_kdt.offset, hip.HILL_CHUNK]
    assert got == want
    assert T.cv2.offset == T.inv_h.offset + 4 and ctypes.sizeof(T) == 48      # the four fields are appended after inv_h


# ------------------------------------------------------------------------------------------------ the description check
def good_desc(hip):
    assert hasattr(hip.BiasTerm, "n_nodes2") and hasattr(hip.BiasTerm, "inv_h2"), "cvf_bias_term has no 2-D fields"
    return _good_desc(hip)


def _good_desc(hip):
    """A harmonic term on CV 1 and a 5 x 4 grid on (CV 0, CV 1) at float 4 of a table of exactly 4 + 4 * 5 * 4 = 84 floats (the table
    pointer is only compared with NULL and looked at for its alignment)."""
    d = hip.BiasDesc()
    d.n_terms, d.n_table, d.table = 2, 84, 4096
    d.term[0].kind, d.term[0].cv, d.term[0].kappa, d.term[0].center = hip.BIAS_HARMONIC, 1, 1.0, 0.5
    t = d.term[1]
    t.kind, t.cv, t.tab_off, t.n_nodes, t.lo, t.inv_h = hip.BIAS_TABLE, 0, 4, 5, -1.0, 2.0
    t.cv2, t.n_nodes2, t.lo2, t.inv_h2 = 1, 4, 0.25, 4.0
    return d


def _set(**fields):
    def change(d):
        for name, value in fields.items():
            setattr(d.term[1], name, value)
    return change


def _top(field, value):
    def change(d):
        setattr(d, field, value)
    return change


INF, NAN = float("inf"), float("nan")
MALFORMED = [("n_nodes2 == 1", _set(n_nodes2=1), "term[1].n_nodes2 = 1"), ("negative n_nodes2", _set(n_nodes2=-3), "term[1].n_nodes2 = -3"),
             ("cv2 == k", _set(cv2=2), "term[1].cv2 = 2"), ("negative cv2", _set(cv2=-1), "term[1].cv2 = -1"),
             ("cv2 == cv", _set(cv2=0), "term[1].cv2 = 0"), ("NaN lo2", _set(lo2=NAN), "term[1].lo2"), ("infinite lo2", _set(lo2=-INF), "term[1].lo2"),
             ("inv_h2 == 0", _set(inv_h2=0.0), "term[1].inv_h2 = 0"), ("negative inv_h2", _set(inv_h2=-4.0), "term[1].inv_h2 = -4"),
             ("infinite inv_h2", _set(inv_h2=INF), "term[1].inv_h2 = inf"), ("NaN inv_h2", _set(inv_h2=NAN), "term[1].inv_h2"),
             ("tab_off % 4 == 2", _set(tab_off=2), "term[1].tab_off = 2"), ("negative tab_off", _set(tab_off=-4), "term[1].tab_off = -4"),
             ("table overrun by one float", _top("n_table", 83), "n_table = 83"),
             ("4 n1 n2 past 2^31", _set(n_nodes=1 << 20, n_nodes2=1 << 20), "= 4398046511108 floats"),
             ("misaligned table", _top("table", 4096 + 8), "16-byte aligned"), ("NULL table", _top("table", None), "table is NULL"),
             # today's refusals stay, on a 2-D term too
             ("cv == k", _set(cv=2), "term[1].cv = 2"), ("n_nodes == 1", _set(n_nodes=1), "term[1].n_nodes = 1"),
             ("inv_h == 0", _set(inv_h=0.0), "term[1].inv_h = 0"), ("NaN lo", _set(lo=NAN), "term[1].lo")]


def test_bias_check_accepts_a_good_2d_description(hip):
    lib = hip.lib()
    d = good_desc(hip)
    assert d.term[1].tab_off + 4 * 5 * 4 == d.n_table
    assert lib.cvf_cv_bias_check(d, 2) == 1, lib.cvf_last_error().decode()
    d.term[1].cv, d.term[1].cv2 = 1, 0                 # either order of the two CVs
    assert lib.cvf_cv_bias_check(d, 2) == 1, lib.cvf_last_error().decode()


def test_a_1d_table_ignores_the_new_fields(hip):
    """n_nodes2 == 0 is the 1-D table of before, whatever cv2, lo2 and inv_h2 hold - and whatever the table's alignment."""
    lib = hip.lib()
    assert hasattr(hip.BiasTerm, "n_nodes2") and ctypes.sizeof(hip.BiasTerm) == 48, "cvf_bias_term has no 2-D fields"
    d = hip.BiasDesc()
    d.n_terms, d.n_table, d.table = 1, 10, 4096 + 4
    t = d.term[0]
    t.kind, t.cv, t.tab_off, t.n_nodes, t.lo, t.inv_h = hip.BIAS_TABLE, 0, 2, 4, -1.0, 2.0
    t.cv2, t.n_nodes2, t.lo2, t.inv_h2 = -77, 0, NAN, -INF
    assert lib.cvf_cv_bias_check(d, 1) == 1, lib.cvf_last_error().decode()


@pytest.mark.parametrize("name,change,word", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_bias_check_refuses_and_names_the_field(hip, name, change, word):
    lib = hip.lib()
    d = good_desc(hip)
    change(d)
    assert lib.cvf_cv_bias_check(d, 2) == 0, name
    why = lib.cvf_last_error().decode()
    assert word in why and why.startswith("cvf_cv_bias_check"), why


def test_python_vocabulary(hip):
    from colvarsfinder import export
    g = B2.deposit_terms(2, True)
    d, table = export.bias_desc([("table", 1, 0.0, 0.5, [0, 1, 2], [1, 1, 1]), g, {"kind": "table", "cv": 0, "lo": 0.0, "h": 0.5, "n": 3},
                                 dict(g, kind="table2d", n=(3, 2), cv=1, cv2=0)], 2)
    assert [d.term[t].tab_off for t in range(4)] == [0, 8, 88, 96] and d.n_table == 96 + 24     # (6 -> 8 and 94 -> 96: multiples of 4)
    assert table.data_ptr() % 16 == 0 and d.table == table.data_ptr()
    e = d.term[1]
    assert (e.kind, e.cv, e.cv2, e.n_nodes, e.n_nodes2, e.lo, e.lo2, e.inv_h, e.inv_h2) == (hip.BIAS_TABLE, 0, 1, 5, 4, -0.5, 0.25, 4.0, 2.0)
    nodes = table[8:88].reshape(5, 4, 4).numpy()
    for c, key in enumerate(("u", "d1", "d2", "d12")):
        assert np.array_equal(nodes[:, :, c], np.float32(g[key]))
    assert (table[6:8] == 0).all() and (table[88:] == 0).all() and (d.term[3].n_nodes, d.term[3].n_nodes2) == (3, 2)
    with pytest.raises(ValueError, match="cv2 = 0"):
        export.bias_desc([dict(g, cv2=0)], 2)
    with pytest.raises(ValueError, match="one shape"):
        export.bias_desc([dict(g, d12=np.zeros((4, 5)))], 2)


# ------------------------------------------------------------------------------------------------ the 2-D formulas on the host
GRID = B2.deposit_terms(2, True)                                   # 5 x 4 nodes: x -0.5 .. 0.5 (h 0.25), y 0.25 .. 1.75 (h 0.5)
XS = [B2.GRID_LO[0] + B2.GRID_H[0] * j for j in range(B2.N1)]
YS = [B2.GRID_LO[1] + B2.GRID_H[1] * j for j in range(B2.N2)]
# below, inside (two different cells) and above, per axis: all nine regions, and more than one cell
NODES1 = [B2.LO1 + B2.H1 * j for j in range(6)]
PX, PY = [-1.3, -0.41, 0.13, 0.38, 0.9], [-0.6, 0.4, 1.1, 1.6, 2.9]
REGION_POINTS = np.array([(x, y) for x in PX for y in PY], dtype=np.float32)


def neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def test_nodes_come_back_bit_for_bit(program):
    """On every node - the last row and column included - U, both slopes and the mixed derivative are the node's four floats."""
    pts = np.array([(x, y) for x in XS for y in YS], dtype=np.float32)
    P, _, _ = program([GRID], 2, pts)
    want = B2.term_nodes(GRID).reshape(-1, 4).astype(np.float32)
    assert P.shape == (20, 4)
    assert np.array_equal(P.astype(np.float32), want)


def test_all_nine_regions_match_fp64(program):
    """U and both gradient components against the fp64 reference; max abs error / the reference's max abs.  The bar: 16 eps, the
    1-D host test's - a bicubic is a few more fp32 operations on numbers of order 1.  Measured: DESIGN.md section 4.19."""
    P, _, _ = program([GRID], 2, REGION_POINTS)
    U64, dU64 = B2.ref_u_du([GRID], REGION_POINTS.astype(np.float64))
    regions = {B2.region(GRID, p)[0] for p in REGION_POINTS.astype(np.float64)}
    assert len(regions) == 9
    eu, ed = np.abs(P[:, 0] - U64).max() / np.abs(U64).max(), np.abs(P[:, 1:3] - dU64).max() / np.abs(dU64).max()
    print(f"[cvbias2] host nine regions: U {eu / EPS:.2f} eps, dU {ed / EPS:.2f} eps")
    assert eu <= 16 * EPS and ed <= 16 * EPS


def test_gradient_is_the_gradient_of_u(program):
    """Both components against central differences of the fp64 U, on the points not adjacent to a cell edge (the kinks of the
    second derivatives).  Step 1e-5: good to 1e-10 |U'''| / 6 plus 1e-16 / 1e-5."""
    P, _, _ = program([GRID], 2, REGION_POINTS)
    x = REGION_POINTS.astype(np.float64)
    step = 1e-5
    smooth = (np.abs(x[:, 0:1] - np.array(XS)[None, :]).min(axis=1) > 10 * step) & (np.abs(x[:, 1:2] - np.array(YS)[None, :]).min(axis=1) > 10 * step)
    assert smooth.sum() >= 20
    _, dU64 = B2.ref_u_du([GRID], x)
    for a in (0, 1):
        e = np.zeros(2)
        e[a] = step
        cd = (B2.ref_u_du([GRID], x + e)[0] - B2.ref_u_du([GRID], x - e)[0]) / (2 * step)
        assert np.abs(P[smooth, 1 + a] - cd[smooth]).max() / np.abs(dU64).max() <= 16 * EPS + 1e-9


def test_u_and_gradient_are_continuous_across_every_node_line_and_edge(program):
    """C1: at the fp32 numbers on either side of every node line (the four grid edges are the first and last of them), U and both
    gradient components differ by no more than slope (curvature) x step plus rounding - along lines that cross the other axis below,
    inside and above the grid."""
    pts = np.array([(n, o) if axis == 0 else (o, n)
                    for axis, lines, across in ((0, XS, [-0.6, 0.25, 0.9, 1.75, 2.9]), (1, YS, [-1.3, -0.5, 0.13, 0.5, 0.9]))
                    for v in lines for o in across for n in neighbours(v)], dtype=np.float32)
    P, _, _ = program([GRID], 2, pts)
    assert len(pts) == 3 * 5 * (B2.N1 + B2.N2)
    for trio, got in zip(pts.reshape(-1, 3, 2), P.reshape(-1, 3, 4)):
        step = float(np.abs(trio[2] - trio[0]).max())
        size_u, size_d = max(1.0, np.abs(got[:, 0]).max()), max(1.0, np.abs(got[:, 1:3]).max())     # rounding: 16 eps of the numbers in play
        assert np.abs(np.diff(got[:, 0])).max() <= 8.0 * step + 16 * EPS * size_u, (trio, got)
        assert np.abs(np.diff(got[:, 1:3], axis=0)).max() <= 16.0 * step + 16 * EPS * size_d, (trio, got)


def test_nan_takes_the_below_branch_and_reads_inside_the_table(program):
    """A NaN coordinate takes the "below" branch of its axis: P sits on the FIRST node line, d = NaN.  U and the slope along the
    other axis are then NaN, but the slope along the NaN axis itself is d_aU(P) + d12U(P) d_other with d_other = 0: finite, and
    the value every point below the grid has at that coordinate of the other axis - not the one above the grid (the last node
    line's), which the test shows to differ.  No read outside the table (the sanitizer watches)."""
    P, _, _ = program([GRID], 2, np.array([[np.nan, 0.9], [0.38, np.nan], [np.nan, np.nan]], dtype=np.float32))
    assert np.isnan(P[:, 0]).all() and np.isnan(P[0, 2]) and np.isnan(P[1, 1]) and np.isnan(P[2, 1:3]).all()
    _, below = B2.ref_u_du([GRID], np.float32([[-1.3, 0.9], [0.38, -0.6]]).astype(np.float64))
    _, above = B2.ref_u_du([GRID], np.float32([[0.9, 0.9], [0.38, 2.9]]).astype(np.float64))
    for row, axis in ((0, 0), (1, 1)):
        assert abs(P[row, 1 + axis] - below[row, axis]) <= 16 * EPS * np.abs(below).max(), (row, P[row], below[row])
        assert abs(above[row, axis] - below[row, axis]) > 0.05                           # (the two branches are told apart)


def test_a_2d_term_and_1d_terms_sum_in_term_order(program):
    """k = 3: a grid on (CV 2, CV 0) between 1-D terms on both of its CVs; bias_torch - the three-call route's twin - agrees."""
    from colvarsfinder import export
    terms = [{"kind": "harmonic", "cv": 2, "kappa": 0.8, "center": -0.2}, dict(GRID, cv=2, cv2=0), Bc.smooth_table(0, -0.75, 4.0, 6, 0.1),
             {"kind": "linear", "cv": 1, "kappa": 0.3}, {"kind": "upper_wall", "cv": 0, "kappa": 2.0, "center": 0.0}]
    xi = np.random.RandomState(3).uniform(-1, 2, size=(24, 3)).astype(np.float32)
    P, _, _ = program(terms, 3, xi)
    U64, dU64 = B2.ref_u_du(terms, xi.astype(np.float64))
    assert np.abs(P[:, 0] - U64).max() <= 16 * EPS * np.abs(U64).max()
    assert np.abs(P[:, 1:4] - dU64).max() <= 16 * EPS * np.abs(dU64).max()
    d, table = export.bias_desc(terms, 3)
    Ut, dUt = export.bias_torch(d, table, torch.tensor(xi))
    assert np.abs(Ut.numpy() - P[:, 0]).max() <= 16 * EPS * np.abs(U64).max()
    assert np.abs(dUt.numpy() - P[:, 1:4]).max() <= 16 * EPS * np.abs(dU64).max()


# ------------------------------------------------------------------------------------------------ deposit on the host
def _term_table(terms, k, index):
    """(offset, floats) of term `index` in the table export.bias_desc lays out."""
    d, _ = B2.layout_of(terms, k)
    e = d.term[index]
    return e.tab_off, (4 * e.n_nodes * e.n_nodes2 if e.n_nodes2 else 2 * e.n_nodes)


@pytest.mark.parametrize("inv_kdt", [0.0, 0.8], ids=["plain", "well-tempered"])
@pytest.mark.parametrize("dim", [1, 2])
def test_deposit_matches_fp64(program, dim, inv_kdt):
    """Three hills - inside, outside the grid, a NaN centre - onto smooth nodes, twice: every height from the table before its call
    (the reference follows that rule), the second call sees the first call's hills.  Table and hills against fp64."""
    term = B2.deposit_terms(dim, True)
    k, centres = (1, B2.HILLS_1D) if dim == 1 else (2, B2.HILLS_2D)
    sigma = (0.3, 0.0) if dim == 1 else (0.3, 0.55)
    call = (0, 1.2, sigma[0], sigma[1], inv_kdt, centres)
    _, H, T = program([term], k, deposits=[call, call])
    nodes0 = B2.nodes_of(term)
    sig = sigma[0] if dim == 1 else sigma
    nodes1, hills1 = B2.ref_deposit(term, nodes0, np.float32(centres), 1.2, sig, inv_kdt)
    nodes2, hills2 = B2.ref_deposit(term, nodes1, np.float32(centres), 1.2, sig, inv_kdt)
    assert H.shape == (6, 4) and T.shape == (nodes0.size,)
    for got, want in ((H[:3], hills1), (H[3:], hills2)):
        assert got[2, 2] == 0.0 and np.isnan(got[2, 0])                            # the NaN hill: w = 0
        assert np.array_equal(got[:2, :2], want[:2, :2])                           # the centres themselves
        assert np.abs(got[:2, 2:] - want[:2, 2:]).max() <= B2.DEP_TOL * np.abs(want[:2, 2:]).max()
    if inv_kdt > 0:
        assert hills2[0, 2] < hills1[0, 2] and H[3, 2] < H[0, 2]                   # the second call's heights saw the first call's hills
    err = B2.rel_cols(T.reshape(nodes2.shape), nodes2)
    print(f"[cvbias2] host deposit {dim}-D inv_kdt {inv_kdt}: table {err / EPS:.2f} eps")
    assert err <= B2.DEP_TOL
    assert np.abs(nodes2 - nodes0).max() > 0.5


@pytest.mark.parametrize("dim", [1, 2])
def test_a_nan_hill_leaves_every_bit(program, dim):
    term = B2.deposit_terms(dim, True)
    k = dim
    row = [B2.NANF] if dim == 1 else [0.1, B2.NANF]
    _, H, T = program([term], k, deposits=[(0, 1.2, 0.3, 0.4, 0.5, [row])])
    _, T0 = B2.layout_of([term], k)
    assert np.array_equal(T.astype(np.float32).view(np.int32), T0.view(np.int32)) and H[0, 2] == 0.0


@pytest.mark.parametrize("dim", [1, 2])
def test_a_weight_that_overflows_is_skipped(program, dim):
    """Well-tempered on a table whose value at the centre is -400 with inv_kdt = 1: exp(400) is past fp32, the row says w = 0 and
    no node changes - none turns NaN (inf x a Gaussian that has underflowed to 0)."""
    term = B2.deposit_terms(dim, False)
    term = dict(term, u=np.full(np.shape(term["u"]), -400.0))
    centre = [0.07] if dim == 1 else [0.07, 0.9]
    _, H, T = program([term], dim, deposits=[(0, 1.2, 0.01, 0.01, 1.0, [centre])])
    _, T0 = B2.layout_of([term], dim)
    assert H[0, 2] == 0.0 and abs(H[0, 3] + 400.0) < 1e-3
    assert np.array_equal(T.astype(np.float32).view(np.int32), T0.view(np.int32))


def test_the_plain_build_prints_the_bits_of_the_sanitized_one(program, tmp_path):
    """tests/test_cv_bias2_gpu.py compares the GPU's table with the program built without sanitizers; here both builds run the
    evaluation points and the deposit cases of that comparison and must agree bit for bit."""
    plain = B2.build_program(tmp_path, sanitize=False)
    for dim in (1, 2):
        term = B2.deposit_terms(dim, True)
        centres = B2.HILLS_1D if dim == 1 else B2.HILLS_2D
        sigma = (0.3, 0.0) if dim == 1 else (0.3, 0.55)
        pts = np.float32(NODES1 + [-2.0, 0.07, 0.8]) if dim == 1 else REGION_POINTS
        for inv_kdt in (0.0, 0.8):
            call = (0, 1.2, sigma[0], sigma[1], inv_kdt, centres)
            a, b = program([term], dim, pts, deposits=[call, call]), plain([term], dim, pts, deposits=[call, call])
            for x, y in zip(a, b):
                assert np.array_equal(x.astype(np.float32).view(np.int32), y.astype(np.float32).view(np.int32)), (dim, inv_kdt)


HILL_REFUSALS = [("term == n_terms", dict(term=3), "hill.term = 3"), ("negative term", dict(term=-1), "hill.term = -1"),
                 ("no table term", dict(term=0), "hill.term = 0"), ("height 0", dict(height=0.0), "hill.height"),
                 ("NaN height", dict(height=NAN), "hill.height"), ("infinite height", dict(height=INF), "hill.height"),
                 ("sigma 0", dict(sigma=0.0), "hill.sigma"), ("infinite sigma", dict(sigma=INF), "hill.sigma"),
                 ("sigma whose 1 / sigma^2 overflows", dict(sigma=1e-20), "1 / sigma^2"), ("sigma2 0 in 2-D", dict(sigma2=0.0), "hill.sigma2"),
                 ("sigma2 whose 1 / sigma2^2 overflows", dict(sigma2=1e-20), "1 / sigma2^2"), ("negative inv_kdt", dict(inv_kdt=-0.5), "hill.inv_kdt"),
                 ("NaN inv_kdt", dict(inv_kdt=NAN), "hill.inv_kdt"), ("another table", dict(table=8192), "bias->table"), ("B < 0", dict(B=-1), "B = -1"),
                 ("NULL xi_rows", dict(xi=None), "null"), ("NULL hills", dict(hills=None), "null")]


@pytest.mark.parametrize("name,change,word", HILL_REFUSALS, ids=[m[0] for m in HILL_REFUSALS])
def test_deposit_refuses_before_any_launch_and_names_the_field(hip, name, change, word):
    """Host arithmetic only: every refusal comes before the first launch, so it can be asked for without a GPU (the pointers are
    never followed).  Term 0 is harmonic, term 1 the 5 x 4 grid, term 2 a 1-D table."""
    lib = hip.lib()
    d = good_desc(hip)
    d.n_terms, d.n_table = 3, 96
    t = d.term[2]
    t.kind, t.cv, t.tab_off, t.n_nodes, t.lo, t.inv_h = hip.BIAS_TABLE, 1, 84, 6, -1.0, 2.0
    assert lib.cvf_cv_bias_check(d, 2) == 1, lib.cvf_last_error().decode()
    h = hip.HillDesc(1, 0, 1.2, 0.3, 0.55, 0.8)
    for field in ("term", "height", "sigma", "sigma2", "inv_kdt"):
        if field in change:
            setattr(h, field, change[field])
    rc = lib.cvf_cv_bias_deposit(d, 2, h, change.get("xi", 4096), change.get("B", 3), change.get("table", 4096), change.get("hills", 4096), None)
    why = lib.cvf_last_error().decode()
    assert rc == -1 and word in why and why.startswith("cvf_cv_bias_deposit"), (name, rc, why)


@pytest.mark.parametrize("ratio", [1.0, 1.5, 2.0, 3.0])
def test_one_hill_on_a_zero_table_interpolates_its_gaussian(program, ratio):
    """1-D, sigma = ratio x h, one hill on a zero table, the centre anywhere in a cell: the interpolated U differs from the analytic
    Gaussian by at most w (h / sigma)^4 / 128 and U' by at most (sqrt(3) / 72) w h^3 / sigma^4 - the cubic-Hermite error bounds
    h^4 max|f''''| / 384 and sqrt(3) h^3 max|f''''| / 216 with max|f''''| = 3 w / sigma^4 - plus fp32 rounding (16 eps of w and of
    the largest slope w / (sigma sqrt(e)))."""
    h, w = B2.H1, 1.2
    sigma = ratio * h
    empty = B2.deposit_terms(1, False)
    n = 6
    x = np.linspace(B2.LO1, B2.LO1 + (n - 1) * h, 241).astype(np.float32)
    for c in (-0.125, -0.07, 0.0, 0.11):                # mid-cell, anywhere, on a node, anywhere
        _, H, T = program([empty], 1, deposits=[(0, w, sigma, 0.0, 0.0, [[c]])])
        assert H[0, 2] == np.float32(w) and H[0, 3] == 0.0
        P, _, _ = program([empty], 1, x, table=T)
        s32, c32 = float(np.float32(sigma)), float(np.float32(c))
        g = w * np.exp(-0.5 * (x.astype(np.float64) - c32) ** 2 / s32 ** 2)
        dg = -g * (x.astype(np.float64) - c32) / s32 ** 2
        eu, ed = np.abs(P[:, 0] - g).max(), np.abs(P[:, 1] - dg).max()
        bu, bd = w * (h / sigma) ** 4 / 128, np.sqrt(3.0) / 72 * w * h ** 3 / sigma ** 4
        print(f"[cvbias2] sigma / h = {ratio}, c = {c}: U {eu / bu:.3f} of its bound, U' {ed / bd:.3f} of its bound")
        assert eu <= bu + 16 * EPS * w and ed <= bd + 16 * EPS * w / (sigma * np.sqrt(np.e))


# ------------------------------------------------------------------------------------------------ the deposit kernels
def test_kernel_resources(tmp_path):
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "cv_bias_hills.o"), tmp_path)
    assert sum("hill_heights_kernel" in n for n in kernels) == 1 and sum("hill_nodes_kernel" in n for n in kernels) == 2, list(kernels)
    for name, r in kernels.items():
        print(f"[cvbias2] {name}: {r['vgpr_count']} VGPRs")
        assert r["vgpr_count"] <= 128, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
