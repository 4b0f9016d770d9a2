"""CPU: the front-kernel instances that read their resident batch's feature tile (csrc/ef16_front_rows.hip), from the built objects.

* every ROWS twin at <= 128 VGPRs; the benchmarked <20, 3, 6, true, true> one without scratch and with no more VGPRs than the
  same instance had before it read the tile (111, measured from the object of the commit before this change - a literal, not a
  figure taken from this tree);
* the entry that fills rows and tile in one launch (cvf_ef16_align_rows_tile): exported, declared in include/cvf.h, bound in
  _hip._SIGNATURES with the arguments of cvf_ef16_align_rows plus the tile in front of the stream; the single filling kernel
  keeps its name.
"""
import ctypes
import os
import re

import pytest

from tests.codeobj import ROOT, built_objects, kernels_of, template_args

VGPR_BEFORE = 111   # ef16_front_kernel<20, 3, 6, true, true> of the parent commit's ef16_front_rows.o


@pytest.fixture(scope="module")
def rows_obj(tmp_path_factory):
    return kernels_of(os.path.join(built_objects(), "ef16_front_rows.o"), tmp_path_factory.mktemp("ef16_front_rows_o"))


def test_rows_twins_fit_the_register_budget(rows_obj):
    twins = {template_args(n, "ef16_front_kernel"): v for n, v in rows_obj.items() if template_args(n, "ef16_front_kernel")}
    assert len(twins) == 192 and all(key[4] == 1 for key in twins)
    for key, v in twins.items():
        assert v["vgpr_count"] <= 128, (key, v)
    c3 = twins[(20, 3, 6, 1, 1)]
    assert c3.get("private_segment_fixed_size", 0) == 0 and c3.get("vgpr_spill_count", 0) == 0, c3
    assert c3["vgpr_count"] <= VGPR_BEFORE, c3


def test_one_filling_kernel(rows_obj):
    assert sum("ef16_align_rows_kernel" in n for n in rows_obj) == 1, sorted(rows_obj)[:3]


def test_fill_entry_is_exported_declared_and_bound():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "colvars-finder_amd"))
    from colvarsfinder import _hip
    built_objects()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(_hip.LIB_PATH)
    name = "cvf_ef16_align_rows_tile"
    assert name in declared and name in _hip._SIGNATURES and hasattr(handle, name)
    a, b = _hip._SIGNATURES["cvf_ef16_align_rows"], _hip._SIGNATURES[name]
    assert b[0] is a[0] and list(b[1]) == list(a[1][:-1]) + [ctypes.c_void_p, a[1][-1]]
