"""CPU: code-object metadata of the kernels of a feature layer without alignment (csrc/k1_features.hip), read from the built
object like tests/test_kernel_resources.py: no scratch, registers that leave two 256-thread workgroups per SIMD set, and an LDS
image that stays within the 160 KB of a CU at the limits include/cvf.h documents."""
import os
import re

from tests.test_kernel_resources import CSRC, built, kernels_of  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(CSRC))
KERNELS = ("features_fwd_kernel", "features_vjp_kernel", "features_metric_kernel")


def test_features_kernels_budget(built, tmp_path):  # noqa: F811
    ks = kernels_of(os.path.join(built, "k1_features.o"), tmp_path)
    for family in KERNELS:
        mine = {n: v for n, v in ks.items() if family in n}
        assert len(mine) == 1, (family, sorted(ks))
        for n, v in mine.items():
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v["vgpr_count"] <= 128, (n, v)


def test_lds_at_the_documented_limits():
    header = open(os.path.join(ROOT, "include", "cvf.h")).read()
    lim = {k: int(v) for k, v in re.findall(r"#define CVF_FEATURES_MAX_(SLOT|REF) (\d+)", header)}
    assert set(lim) == {"SLOT", "REF"}
    # one frame and one net per workgroup at the limits: feature atoms (12 B), contribution rows (12 B), the metric kernel's 8 KB
    # of per-wave energy sums
    assert 12 * lim["SLOT"] + 12 * lim["REF"] + 8 * 1024 <= 160 * 1024
    # the lists the issue names: config 5 (128 dihedrals + 128 bonds: 768 atoms, 768 rows) and 64 positions
    assert lim["SLOT"] >= 768 and lim["REF"] >= 768
