"""CPU: register budget of the factored-metric kernel (csrc/metric_factor.hip), read from the built code object like
tests/test_kernel_resources.py.  Its design rests on several 256-thread workgroups per CU keeping their staged records in flight:
at most 96 VGPRs (five waves per SIMD by registers) and no scratch."""
import os

from tests.test_kernel_resources import CSRC, built, kernels_of  # noqa: F401  (fixture)


def test_metric_factor_kernel_budget(built, tmp_path):  # noqa: F811
    ks = kernels_of(os.path.join(built, "metric_factor.o"), tmp_path)
    mk = {n: v for n, v in ks.items() if "metric_factor_kernel" in n}
    fk = {n: v for n, v in ks.items() if "k1_factor_kernel" in n}
    assert len(mk) == 1 and len(fk) == 1
    for n, v in list(mk.items()) + list(fk.items()):
        assert v["vgpr_count"] <= 96, (n, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
