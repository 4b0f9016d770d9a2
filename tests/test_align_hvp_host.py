"""CPU: the Hessian-vector product of the alignment + feature layer - ``cvf_align_feature_hvp`` is declared, bound and exported,
its kernels are the five DESIGN.md 4.14 names with the resources it records (read from the code object `make` built, as
tests/test_align_jvp_host.py does), ``second_order="complete"`` is an accepted option, and the closed form the kernels evaluate
for the rigid-body part agrees with fp64 autograd through the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.codeobj import CSRC, LLVM, built_objects, kernels_of

ROOT = os.path.dirname(os.path.dirname(CSRC))
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def built():
    return built_objects()


def test_hvp_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cvf.h")).read()
    assert re.search(r"\bint cvf_align_feature_hvp\(const cvf_pp_desc\* pp, const float\* x, int64_t B, const float\* aux_tiled,\s*"
                     r"const float\* g_rows, const float\* u_rows, float\* h_rows, void\* stream\);", header)
    from colvarsfinder import _hip
    assert "cvf_align_feature_hvp" in _hip.EXPORTED_SYMBOLS
    res, args = _hip._SIGNATURES["cvf_align_feature_hvp"]
    vres, vargs = _hip._SIGNATURES["cvf_align_feature_vjp"]
    assert res == vres and args == vargs[:5] + vargs[4:]   # the VJP's list with one more row pointer (g_rows, u_rows, h_rows)
    assert _hip.lib().cvf_align_feature_hvp is not None   # (lib() binds every declared symbol and raises on a missing one)


def test_hvp_kernels_and_their_resources(built, tmp_path):
    ks = kernels_of(os.path.join(built, "k1_hvp.o"), tmp_path)
    small = {n: v for n, v in ks.items() if "hvp_align_kernel" in n}
    large = {n: v for n, v in ks.items() if "hvp_large_kernel" in n}
    feat = {n: v for n, v in ks.items() if "features_hvp_kernel" in n}
    # <tables in LDS> or not; uniform and weighted; one kernel without alignment - and nothing else in the object
    assert len(small) == 2 and len(large) == 2 and len(feat) == 1 and len(ks) == 5, sorted(ks)
    for n in ks:   # the guards of k1_vjp.o / k1_jvp.o / k1_features.o match on these substrings
        assert not any(tag in n for tag in ("vjp_", "jvp_", "features_jvp", "features_vjp")), n
    for n, v in ks.items():
        assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
    # the finished build reports 120 / 120 (lane per frame), 107 / 107 (workgroup per frame) and 64 (no alignment)
    for n, v in small.items():   # as vjp_align_kernel: the LDS images allow a few waves per CU, 128 registers leave four per SIMD
        assert v["vgpr_count"] <= 120, (n, v)
    for n, v in large.items():   # 4 waves per workgroup, 128 registers = 4 workgroups per CU
        assert v["vgpr_count"] <= 107, (n, v)
    for n, v in feat.items():    # 64 registers: 8 waves per SIMD
        assert v["vgpr_count"] <= 64, (n, v)
    # LDS: the static part from the code object (kernels_of left it in tmp_path), the dynamic part as the host sizes it
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(tmp_path / "x.co")], check=True, capture_output=True, text=True).stdout
    static = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    assert len(static) == 5 and max(static) <= 1024, static
    stride = lambda nc: nc if nc % 4 == 2 else nc | 1   # x_tile_stride (csrc/cvf_common.hpp)
    assert max(3 * 64 * stride(nc) * 4 for nc in range(9, 193, 3)) == 148224 <= LDS_LIMIT   # x, u, h images at 192 coordinates
    # (a large frame's rows, n_ref * 12 bytes plus the static part, are checked against the limit by the call itself)
    from colvarsfinder import _hip
    assert (_hip.FEATURES_MAX_SLOT + _hip.FEATURES_MAX_REF) * 12 <= LDS_LIMIT   # no alignment at the limits: u stays in memory


def test_second_order_complete_is_an_option():
    from colvarsfinder import pp
    assert pp._SECOND_ORDER == (None, "cotangent", "complete")
    feats = [("position", (0, 1, 2, 3))]
    ref = np.random.RandomState(0).randn(4, 3)
    layer = pp.AlignFeatureLayer(4, [0, 1, 2, 3], ref, feats, second_order="complete")
    assert layer.second_order == "complete"
    layer.second_order = "cotangent"
    layer.second_order = "complete"
    layer.second_order = None
    with pytest.raises(ValueError, match="second_order"):
        layer.second_order = "full"
    with pytest.raises(ValueError, match="second_order"):
        pp.AlignFeatureLayer(4, [0, 1, 2, 3], ref, feats, second_order="full")
    assert "complete" in pp._NO_DOUBLE_BACKWARD and "third derivatives" in pp._NO_THIRD_ORDER


@pytest.mark.parametrize("weighted", [False, True])
def test_closed_form_of_the_rigid_body_part_vs_fp64_autograd(weighted):
    from oracle.pp import AlignFeature
    from tests.align_hvp_cases import double_backward, rigid_hvp_np
    rs = np.random.RandomState(3 + weighted)
    N, al, pos = 12, [0, 2, 3, 5, 7, 8, 11], [1, 2, 4, 5, 9, 11]
    ref = rs.randn(len(al), 3)
    w = rs.uniform(0.2, 3.0, size=len(al)) if weighted else None
    frames = rs.randn(3, N, 3)
    for x in frames:   # roughly a rotated, shifted, noisy copy of the reference on the align atoms
        x[al] = ref @ np.linalg.qr(rs.randn(3, 3))[0] + 0.2 * rs.randn(len(al), 3) + 1.5
    g, u = rs.randn(3, len(pos), 3), rs.randn(3, N, 3)
    torch.set_default_dtype(torch.float64)
    try:
        f = AlignFeature(al, ref, [("position", tuple(pos))], align_weights=w)
        _, want = double_backward(f, torch.tensor(frames), torch.tensor(g).reshape(3, -1), torch.tensor(u))
    finally:
        torch.set_default_dtype(torch.float32)
    want = want.numpy()
    for b in range(3):
        got = rigid_hvp_np(frames[b], al, ref, pos, g[b], u[b], weights=w)
        err = np.abs(got - want[b]).max() / np.abs(want[b]).max()
        assert err <= 1e-10, (b, err)
