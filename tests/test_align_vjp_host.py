"""CPU: the VJP entry point of the alignment + feature layer is declared, exported, and its kernels keep the register budget
DESIGN.md 4.6 states (read from the code object `make` built, as tests/test_kernel_resources.py does)."""
import os
import subprocess

import pytest

from tests.test_kernel_resources import CSRC, LLVM, kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "colvars-finder_amd", "colvarsfinder", "libcvf_hip.so")


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    return os.path.join(CSRC, "build")


def test_vjp_symbol_is_declared_and_exported(built):
    from colvarsfinder import _hip
    assert "cvf_align_feature_vjp" in _hip.EXPORTED_SYMBOLS
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not in this image")
    table = subprocess.run([readelf, "--dyn-syms", "--wide", LIB], check=True, capture_output=True, text=True).stdout
    defined = {f[-1] for f in (line.split() for line in table.splitlines()) if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND"}
    assert "cvf_align_feature_vjp" in defined


def test_vjp_kernels_keep_their_budget(built, tmp_path):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not in this image")
    ks = kernels_of(os.path.join(built, "k1_vjp.o"), tmp_path)
    small = {n: v for n, v in ks.items() if "vjp_align_kernel" in n}
    large = {n: v for n, v in ks.items() if "vjp_large_kernel" in n}
    assert len(small) == 2 and len(large) == 2, sorted(ks)
    for n, v in list(small.items()) + list(large.items()):
        assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
    # lane per frame: the LDS (two 64-frame images) allows at most a few waves per CU - 128 registers leave four per SIMD
    for n, v in small.items():
        assert v["vgpr_count"] <= 128, (n, v)
    # workgroup per frame, 4 waves: 64 registers = 8 waves per SIMD = 8 workgroups per CU in flight, whose gathers (phase A)
    # and table lookups (phase 2) overlap the stores of the others
    for n, v in large.items():
        assert v["vgpr_count"] <= 64, (n, v)
