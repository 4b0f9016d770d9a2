"""CPU: the front-kernel instances that start from alignment rows (csrc/ef16_front_rows.hip), read from the built objects.

* one ROWS twin per generator instance of ef16_front.o - 16 (H, NH) x NIT 1..6 x ALLAL = 192, so a missing (H, NH, NIT, ALLAL)
  is red - and no transfer-operator (NIT = 0) twin;
* every twin at <= 128 VGPRs (3.7 waves per SIMD), the benchmarked <20, 3, 6, true> one without scratch and with no
  more registers than the instance that solves (it does strictly less);
* the new C-ABI entry points: declared in include/cvf.h, bound in _hip._SIGNATURES, exported by the library - all three agree.
"""
import ctypes
import os
import re

import pytest

from tests import ef_cases as E
from tests.codeobj import CSRC, ROOT, built_objects, kernels_of, template_args

NEW = ("cvf_ef16_align_rows_floats", "cvf_ef16_align_rows", "cvf_ef16_front_rows")


@pytest.fixture(scope="module")
def fronts(tmp_path_factory):
    built = built_objects()
    out = {}
    for obj in ("ef16_front.o", "ef16_front_rows.o"):
        ks = kernels_of(os.path.join(built, obj), tmp_path_factory.mktemp(obj.replace(".", "_")))
        out[obj] = {template_args(n, "ef16_front_kernel"): v for n, v in ks.items() if template_args(n, "ef16_front_kernel")}
        out[obj + ":all"] = ks
    return out


def test_one_rows_twin_per_generator_instance(fronts):
    solving, rows = fronts["ef16_front.o"], fronts["ef16_front_rows.o"]
    assert all(len(key) == 5 and key[4] == 1 for key in rows), sorted(rows)[:3]          # <H, NH, NIT, ALLAL, ROWS = true>
    assert all(len(key) == 5 and key[4] == 0 for key in solving), sorted(solving)[:3]
    want = {(H, NH, nit, allal) for H, NH in E.EF16_SHAPES for nit in range(1, 7) for allal in (0, 1)}
    assert len(want) == 192
    assert {key[:4] for key in rows} == want
    assert {key[:4] for key in solving} == want | {(H, NH, 0, 1) for H, NH in E.EF16_SHAPES}
    assert any("ef16_align_rows_kernel" in n for n in fronts["ef16_front_rows.o:all"])   # the single filling kernel


def test_rows_twins_keep_the_occupancy(fronts):
    solving, rows = fronts["ef16_front.o"], fronts["ef16_front_rows.o"]
    for key, v in rows.items():
        assert v["vgpr_count"] <= 128, (key, v)
    c3, c3_solving = rows[(20, 3, 6, 1, 1)], solving[(20, 3, 6, 1, 0)]
    assert c3.get("private_segment_fixed_size", 0) == 0, c3
    assert c3["vgpr_count"] <= c3_solving["vgpr_count"], (c3, c3_solving)


def test_header_binding_and_exports_agree():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "colvars-finder_amd"))
    from colvarsfinder import _hip
    built_objects()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(_hip.LIB_PATH)
    exported = {name for name in declared | set(_hip._SIGNATURES) if hasattr(handle, name)}
    for name in NEW:
        assert name in declared and name in _hip._SIGNATURES and name in exported and hasattr(handle, name), name
    assert set(_hip._SIGNATURES) == declared                       # binding <-> header, both directions
    assert declared <= exported, sorted(declared - exported)       # header -> library
    # the twin takes cvf_ef16_front's arguments + the rows in front of the stream
    a, b = _hip._SIGNATURES["cvf_ef16_front"], _hip._SIGNATURES["cvf_ef16_front_rows"]
    assert b[0] is a[0] and list(b[1]) == list(a[1][:-1]) + [ctypes.c_void_p, a[1][-1]]
    assert os.path.exists(os.path.join(CSRC, "ef16_front_rows.hip"))
