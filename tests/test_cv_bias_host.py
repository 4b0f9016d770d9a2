"""CPU: the bias entry points' ABI, the description check, the predicates against their namesakes, the new kernels' resources, and
the term formulas of csrc/cvf_bias.hpp - compiled into the stand-alone host program tools/bias_host.cpp (with
-fsanitize=address,undefined, a plain executable) - against the fp64 definitions of tests/cv_bias_cases.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import cv_bias_cases as Bc
from tests import cv_frame_cases as F
from tests import cv_frame_large_cases as G

NEW = ("cvf_cv_bias_check", "cvf_cv_frame_bias_supported", "cvf_cv_frame_bias_eval", "cvf_cv_frame_bias_shared_supported",
       "cvf_cv_frame_bias_shared_eval", "cvf_cv_frame_large_bias_supported", "cvf_cv_frame_large_bias_eval",
       "cvf_cv_frame_large_bias_shared_supported", "cvf_cv_frame_large_bias_shared_eval")
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_declared_bound_and_defined(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert set(hip._SIGNATURES) == declared


def test_struct_sizes_match_the_header(hip, tmp_path):
    """sizeof and the offset of the last field, as the C compiler lays the header's structs out."""
    cc = f"{codeobj.LLVM}/clang"
    assert os.path.exists(cc), f"{cc}: the toolchain that builds the library is missing"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cvf.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(cvf_bias_term), sizeof(cvf_bias_desc), offsetof(cvf_bias_desc, table), sizeof(cvf_md_layout), "
                   "offsetof(cvf_md_layout, x_frame_stride), offsetof(cvf_md_layout, f_frame_stride), CVF_BIAS_MAX_TERMS); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I" + os.path.join(codeobj.ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.split()]
    want = [ctypes.sizeof(hip.BiasTerm), ctypes.sizeof(hip.BiasDesc), hip.BiasDesc.table.offset, ctypes.sizeof(hip.MDLayout),
            hip.MDLayout.x_frame_stride.offset, hip.MDLayout.f_frame_stride.offset, hip.BIAS_MAX_TERMS]
    assert got == want
    assert (hip.BIAS_HARMONIC, hip.BIAS_UPPER_WALL, hip.BIAS_LOWER_WALL, hip.BIAS_LINEAR, hip.BIAS_TABLE) == (0, 1, 2, 3, 4)


# ------------------------------------------------------------------------------------------------ the description check
def good_desc(hip, n_table=12):
    """A harmonic term on CV 1 and a 4-node table on CV 0 over 12 floats (the table pointer is only compared with NULL)."""
    d = hip.BiasDesc()
    d.n_terms, d.n_table, d.table = 2, n_table, 16
    d.term[0].kind, d.term[0].cv, d.term[0].kappa, d.term[0].center = hip.BIAS_HARMONIC, 1, 1.0, 0.5
    t = d.term[1]
    t.kind, t.cv, t.tab_off, t.n_nodes, t.lo, t.inv_h = hip.BIAS_TABLE, 0, 4, 4, -1.0, 2.0
    return d


def _set(field, value, term=1):
    def change(d):
        setattr(d.term[term], field, value)
    return change


def _top(field, value):
    def change(d):
        setattr(d, field, value)
    return change


MALFORMED = [("cv == k", _set("cv", 2), "term[1].cv = 2"), ("n_nodes == 1", _set("n_nodes", 1), "term[1].n_nodes = 1"),
             ("inv_h == 0", _set("inv_h", 0.0), "term[1].inv_h = 0"), ("odd tab_off", _set("tab_off", 3), "term[1].tab_off = 3"),
             ("table overrun by one float", _top("n_table", 11), "n_table = 11"),
             ("NaN kappa", _set("kappa", float("nan"), term=0), "term[0].kappa"), ("n_terms == 17", _top("n_terms", 17), "n_terms = 17"),
             ("table term with a NULL table", _top("table", None), "table is NULL"),
             ("unknown kind", _set("kind", 5), "term[1].kind = 5"), ("negative cv", _set("cv", -1), "term[1].cv = -1"),
             ("infinite center", _set("center", float("inf"), term=0), "term[0].center"), ("NaN lo", _set("lo", float("nan")), "term[1].lo"),
             ("negative inv_h", _set("inv_h", -2.0), "term[1].inv_h = -2"), ("negative tab_off", _set("tab_off", -2), "term[1].tab_off = -2")]


def test_bias_check_accepts_a_good_description(hip):
    lib = hip.lib()
    assert lib.cvf_cv_bias_check(good_desc(hip), 2) == 1, lib.cvf_last_error().decode()
    empty = hip.BiasDesc()
    assert lib.cvf_cv_bias_check(empty, 1) == 1      # no terms: U = 0
    d = good_desc(hip)
    d.term[1].tab_off = 0                            # 0 + 2 * 4 <= 12, and exactly at the end: 4 + 2 * 4 == 12 above
    assert lib.cvf_cv_bias_check(d, 2) == 1


@pytest.mark.parametrize("name,change,word", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_bias_check_refuses_and_names_the_field(hip, name, change, word):
    lib = hip.lib()
    d = good_desc(hip)
    change(d)
    assert lib.cvf_cv_bias_check(d, 2) == 0, name
    why = lib.cvf_last_error().decode()
    assert word in why and why.startswith("cvf_cv_bias_check"), why


def test_python_terms_raise_value_error_with_the_c_message(hip):
    from colvarsfinder import export
    d, table = export.bias_desc([("harmonic", 1, 1.0, 0.5), ("linear", 0, -2.0),
                                 {"kind": "table", "cv": 0, "lo": -1.0, "h": 0.5, "u": [0, 1, 2, 3], "du": [1, 1, 1, 1]}], 2)
    assert d.n_terms == 3 and d.n_table == 8 and d.term[2].tab_off == 0 and d.term[2].n_nodes == 4 and d.term[2].inv_h == 2.0
    assert table.tolist() == [0, 1, 1, 1, 2, 1, 3, 1]
    with pytest.raises(ValueError, match="cv = 2"):
        export.bias_desc([("harmonic", 2, 1.0, 0.5)], 2)
    with pytest.raises(ValueError, match="n_terms = 17"):
        export.bias_desc([("linear", 0, 1.0)] * 17, 2)
    with pytest.raises(ValueError, match="n_nodes = 1"):
        export.bias_desc([("table", 0, 0.0, 0.5, [1.0], [1.0])], 1)
    with pytest.raises(ValueError, match="kind"):
        export.bias_desc([("parabola", 0, 1.0, 0.5)], 1)


# ------------------------------------------------------------------------------------------------ the predicates
@pytest.mark.parametrize("row", F.predicate_table(), ids=lambda r: r[0])
def test_wave_predicate_follows_its_namesake(hip, row):
    """cvf_cv_frame_bias_supported keeps 2 k more floats of LDS: none of the table's models sits within 64 bytes of the limit."""
    _, m, upto, pp, want, words = row
    lib = hip.lib()
    assert lib.cvf_cv_frame_supported(m, upto, pp) == want
    got = lib.cvf_cv_frame_bias_supported(m, upto, pp)
    why = lib.cvf_last_error().decode()
    assert got == want, why
    if want == 0:
        assert words in why and "three-call recipe" in why and why.startswith("cvf_cv_frame_bias"), why


@pytest.mark.parametrize("row", G.predicate_table(), ids=lambda r: r[0])
def test_workgroup_predicate_follows_its_namesake(hip, row):
    _, m, upto, pp, want, words = row
    lib = hip.lib()
    assert lib.cvf_cv_frame_large_supported(m, upto, pp) == want
    got = lib.cvf_cv_frame_large_bias_supported(m, upto, pp)
    why = lib.cvf_last_error().decode()
    assert got == want, why
    if want == 0:
        assert words in why and "three-call recipe" in why and why.startswith("cvf_cv_frame_large_bias"), why


def shared_desc(hip, d_r=30, k=2):
    """Form C by hand: k chains [d_r, 8, 4, 1] whose first layer is one set of tensors."""
    m = F.mlp([d_r, 8, 4, 1], k)
    for i in range(1, k):
        m.w_off[i][0], m.b_off[i][0] = m.w_off[0][0], m.b_off[0][0]
    return m


def test_shared_predicates_follow_their_namesakes(hip):
    lib = hip.lib()
    m = shared_desc(hip)
    small, large = F.pp_desc(hip.PP_ALIGN, 30, 30), G.pp_large(hip.PP_ALIGN, 195, 30)
    for ns, want in ((1, 1), (0, 0), (3, 0), (2, 0)):    # n_shared = 2: layer 1 is not shared
        assert lib.cvf_cv_frame_shared_supported(m, ns, small) == want
        assert lib.cvf_cv_frame_bias_shared_supported(m, ns, small) == want, lib.cvf_last_error().decode()
        assert lib.cvf_cv_frame_large_shared_supported(m, ns, large) == want
        assert lib.cvf_cv_frame_large_bias_shared_supported(m, ns, large) == want, lib.cvf_last_error().decode()
    assert lib.cvf_cv_frame_bias_shared_supported(m, 0, small) == 0 and "cvf_cv_frame_bias_eval" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_frame_large_bias_shared_supported(m, 0, large) == 0 and "cvf_cv_frame_large_bias_eval" in lib.cvf_last_error().decode()


def test_the_wave_launch_counts_its_seed_row_in_the_64_kib(hip):
    """k = 8 identity chains of seven hidden layers, the width stepped over the limit: the bias launch needs 2 k = 16 floats more
    than its namesake and declines exactly where the mirror of the layout plus those floats passes 64 KiB."""
    lib = hip.lib()
    seen = set()
    for w in range(200, 257):
        m, pp = F.mlp([512] + [w] * 7 + [1], 8), F.pp_desc(hip.PP_IDENTITY, 512, 512)
        fits = 4 * (F.lds_floats(m, 8, pp) + 16) <= 64 * 1024
        assert lib.cvf_cv_frame_bias_supported(m, 8, pp) == int(fits), (w, lib.cvf_last_error().decode())
        seen.add(fits)
    assert seen == {True, False}


def test_kernel_resources(tmp_path):
    """The bounds the namesakes' code objects are held to (tests/test_cv_frame_host.py, tests/test_cv_frame_large_host.py)."""
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "cv_bias.o"), tmp_path)
    assert sum("cv_frame_bias_kernel" in n for n in kernels) == 2 and sum("cv_frame_large_bias_kernel" in n for n in kernels) == 6
    for name, r in kernels.items():
        print(f"[cvbias] {name}: {r['vgpr_count']} VGPRs")
        assert r["vgpr_count"] <= 128, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


# ------------------------------------------------------------------------------------------------ the term formulas on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tools/bias_host.cpp with the address and undefined-behaviour sanitizers, as a plain executable."""
    cxx = f"{codeobj.LLVM}/clang++"
    assert os.path.exists(cxx), f"{cxx}: the toolchain that builds the library is missing"
    exe = str(tmp_path_factory.mktemp("bias") / "bias_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(codeobj.ROOT, "include"), "-I" + codeobj.CSRC, os.path.join(codeobj.ROOT, "tools", "bias_host.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(terms, k, xi):
        """(U [P], dU [P, k]) of the program for term dicts (tests/cv_bias_cases vocabulary) at points xi [P, k] (fp32)."""
        from colvarsfinder import _hip
        xi = np.asarray(xi, dtype=np.float32).reshape(-1, k)
        lines, table = [], []
        for t in terms:
            if t["kind"] == "table":
                u, du = np.float32(t["u"]), np.float32(t["du"])
                lines.append(f"{_hip.BIAS_TABLE} {t['cv']} 0 0 {len(table)} {len(u)} {float(np.float32(t['lo']))!r} {float(np.float32(t['inv_h']))!r}")
                table += [float(v) for pair in zip(u, du) for v in pair]
            else:
                lines.append(f"{_hip.BIAS_KINDS[t['kind']]} {t['cv']} {float(np.float32(t['kappa']))!r} {float(np.float32(t.get('center', 0.0)))!r} 0 0 0 0")
        text = "\n".join([f"{k} {len(terms)} {len(table)} {len(xi)}"] + lines + [" ".join(repr(v) for v in table)]
                         + [" ".join(repr(float(v)) for v in row) for row in xi]) + "\n"
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=60).stdout
        a = np.array([[float(v) for v in line.split()] for line in out.strip().split("\n")])
        assert a.shape == (len(xi), 1 + k)
        return a[:, 0], a[:, 1:]

    return run


def neighbours(x):
    """fp32: x, the two numbers on either side of it."""
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


TABLE = Bc.smooth_table(0, -0.75, 4.0, 6, 0.1)                      # nodes at -0.75, -0.5, .., 0.5
NODES = [-0.75 + 0.25 * j for j in range(6)]
HOST_TERMS = {
    "harmonic": [{"kind": "harmonic", "cv": 0, "kappa": 1.3, "center": 0.2}],
    "upper_wall": [{"kind": "upper_wall", "cv": 0, "kappa": 1.5, "center": 0.2}],
    "lower_wall": [{"kind": "lower_wall", "cv": 0, "kappa": 1.5, "center": 0.2}],
    "linear": [{"kind": "linear", "cv": 0, "kappa": -1.2}],
    "table": [TABLE],
    "three-on-one": [{"kind": "harmonic", "cv": 0, "kappa": 0.7, "center": -0.3}, {"kind": "upper_wall", "cv": 0, "kappa": 1.1, "center": 0.4},
                     {"kind": "lower_wall", "cv": 0, "kappa": 0.9, "center": -0.1}],
}
# below, at and above c (0.2) for the walls; on the first, an inner and the last node, inside intervals, below lo, above the last node
POINTS = sorted(set(float(v) for x in [0.2, -0.3, 0.4, -0.1, NODES[0], NODES[2], NODES[5]] for v in neighbours(x))
                | {-2.0, -0.9, -0.6, -0.33, 0.07, 0.3, 0.45, 0.8, 2.5})


@pytest.mark.parametrize("case", list(HOST_TERMS), ids=lambda c: c)
def test_terms_match_fp64_and_the_derivative_is_the_derivative(program, case):
    """U and U' against the fp64 definitions (U' there by autograd), and U' against a central difference of the fp64 U.
    Bars: U and U' are a handful of fp32 operations on numbers of order 1 - 16 eps of the largest magnitude in play; the central
    difference with step 1e-5 of a piecewise cubic with curvature of order 1 is good to 1e-5^2 * |U'''| / 6 plus 1e-16 / 1e-5."""
    terms = HOST_TERMS[case]
    pts = np.array(POINTS, dtype=np.float32)
    U, dU = program(terms, 1, pts)
    U64, dU64 = Bc.ref_u_du(terms, pts.astype(np.float64)[:, None])
    scale_u, scale_d = max(1.0, np.abs(U64).max()), max(1.0, np.abs(dU64).max())
    eu, ed = np.abs(U - U64).max() / scale_u, np.abs(dU - dU64).max() / scale_d
    print(f"[cvbias] host {case}: U {eu:.2e} dU {ed:.2e}")
    assert eu <= 16 * EPS and ed <= 16 * EPS
    # central difference of the fp64 U, away from the kinks of U'' (the walls' c, the nodes): on the points not adjacent to one
    step = 1e-5
    x = pts.astype(np.float64)
    kinks = np.array([0.2, -0.3, 0.4, -0.1] + NODES)
    smooth = np.abs(x[:, None] - kinks[None, :]).min(axis=1) > 10 * step
    up, _ = Bc.ref_u_du(terms, (x + step)[:, None])
    um, _ = Bc.ref_u_du(terms, (x - step)[:, None])
    cd = (up - um) / (2 * step)
    assert smooth.sum() >= 9
    assert np.abs(dU[smooth, 0] - cd[smooth]).max() / scale_d <= 16 * EPS + 1e-9


def test_u_and_du_are_continuous_across_nodes_ends_and_walls(program):
    """C1: across every node, both ends of the grid and the walls' c, U and U' at the fp32 numbers on either side differ by no more
    than the slope (curvature) times the step plus rounding."""
    for case, where in (("table", NODES), ("upper_wall", [0.2]), ("lower_wall", [0.2]), ("three-on-one", [-0.3, 0.4, -0.1])):
        for x in where:
            pts = np.array(neighbours(x), dtype=np.float32)
            U, dU = program(HOST_TERMS[case], 1, pts)
            step = float(pts[2] - pts[0])
            assert np.abs(np.diff(U)).max() <= 4.0 * step + 8 * EPS, (case, x, U)
            assert np.abs(np.diff(dU[:, 0])).max() <= 8.0 * step + 16 * EPS, (case, x, dU)


def test_last_node_first_node_and_beyond(program):
    """xi exactly on a node gives the node's pair bit for bit (t = 0 or t = 1 of the basis); beyond the ends the line of the end node."""
    u, du = np.float32(TABLE["u"]), np.float32(TABLE["du"])
    U, dU = program([TABLE], 1, np.array(NODES + [-1.75, 1.5], dtype=np.float32))
    assert np.array_equal(U[:6].astype(np.float32), u) and np.array_equal(dU[:6, 0].astype(np.float32), du)
    assert np.float32(dU[6, 0]) == du[0] and np.float32(dU[7, 0]) == du[5]
    np.testing.assert_allclose(U[6], float(u[0]) + float(du[0]) * -1.0, rtol=4 * EPS)
    np.testing.assert_allclose(U[7], float(u[5]) + float(du[5]) * 1.0, rtol=4 * EPS)


def test_terms_on_several_cvs_sum_in_term_order(program):
    terms = [{"kind": "harmonic", "cv": 1, "kappa": 0.8, "center": -0.2}, dict(TABLE, cv=0), {"kind": "linear", "cv": 1, "kappa": 0.3},
             {"kind": "upper_wall", "cv": 2, "kappa": 2.0, "center": 0.0}]
    xi = np.random.RandomState(3).uniform(-1, 1, size=(9, 3)).astype(np.float32)
    U, dU = program(terms, 3, xi)
    U64, dU64 = Bc.ref_u_du(terms, xi.astype(np.float64))
    assert np.abs(U - U64).max() <= 16 * EPS * max(1.0, np.abs(U64).max())
    assert np.abs(dU - dU64).max() <= 16 * EPS * max(1.0, np.abs(dU64).max())


def test_torch_twin_of_the_three_call_route_matches_the_program(program):
    """export.bias_torch (what BiasedCV's three-call route evaluates in fp32) against the program on the same description."""
    from colvarsfinder import export
    terms = [{"kind": "harmonic", "cv": 1, "kappa": 0.8, "center": -0.2}, dict(TABLE, cv=0), {"kind": "lower_wall", "cv": 1, "kappa": 0.3, "center": 0.1},
             {"kind": "upper_wall", "cv": 0, "kappa": 2.0, "center": 0.0}, {"kind": "linear", "cv": 0, "kappa": 0.4}]
    xi = np.concatenate([np.random.RandomState(4).uniform(-1.5, 1.5, size=(20, 2)), [[NODES[5], 0.1], [NODES[0], -0.2], [NODES[3], 0.3]]]).astype(np.float32)
    d, table = export.bias_desc(terms, 2)
    Ut, dUt = export.bias_torch(d, table, torch.tensor(xi))
    U, dU = program(terms, 2, xi)
    assert np.abs(Ut.numpy() - U).max() <= 16 * EPS * max(1.0, np.abs(U).max())
    assert np.abs(dUt.numpy() - dU).max() <= 16 * EPS * max(1.0, np.abs(dU).max())
