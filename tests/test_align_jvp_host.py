"""CPU: the JVP entry point of the alignment + feature layer is declared, bound and exported, and its kernels keep the register
budgets DESIGN.md 4.13 records (read from the code objects `make` built, as tests/test_align_vjp_host.py does)."""
import os
import re

import pytest

from tests.codeobj import CSRC, built_objects, kernels_of

ROOT = os.path.dirname(os.path.dirname(CSRC))


@pytest.fixture(scope="module")
def built():
    return built_objects()


def test_jvp_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cvf.h")).read()
    assert re.search(r"\bint cvf_align_feature_jvp\(const cvf_pp_desc\* pp, const float\* x, int64_t B, const float\* aux_tiled,\s*"
                     r"const float\* u_rows, float\* q_rows, void\* stream\);", header)
    from colvarsfinder import _hip
    assert "cvf_align_feature_jvp" in _hip.EXPORTED_SYMBOLS
    assert _hip._SIGNATURES["cvf_align_feature_jvp"] == _hip._SIGNATURES["cvf_align_feature_vjp"]   # the transpose: same argument list
    assert _hip.lib().cvf_align_feature_jvp is not None   # (lib() binds every declared symbol and raises on a missing one)


def test_jvp_kernels_keep_their_budget(built, tmp_path):
    ks = kernels_of(os.path.join(built, "k1_jvp.o"), tmp_path)
    small = {n: v for n, v in ks.items() if "jvp_align_kernel" in n}
    large = {n: v for n, v in ks.items() if "jvp_large_kernel" in n}
    feat = {n: v for n, v in kernels_of(os.path.join(built, "k1_features.o"), tmp_path).items() if "features_jvp_kernel" in n}
    # <tables in LDS, q image in LDS>, <q image in LDS>, <neither>; uniform and weighted; one kernel without alignment
    assert len(small) == 3 and len(large) == 2 and len(feat) == 1, (sorted(ks), sorted(feat))
    for n, v in list(small.items()) + list(large.items()) + list(feat.items()):
        assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
    # the finished build reports 120 / 120 / 122 (lane per frame), 61 (workgroup per frame) and 47 (no alignment)
    for n, v in small.items():   # as vjp_align_kernel: the LDS images allow a few waves per CU, 128 registers leave four per SIMD
        assert v["vgpr_count"] <= 122, (n, v)
    for n, v in large.items():   # 4 waves per workgroup, 64 registers = 8 workgroups per CU whose gathers overlap
        assert v["vgpr_count"] <= 61, (n, v)
    for n, v in feat.items():
        assert v["vgpr_count"] <= 47, (n, v)
