"""Kernel metadata of the gfx950 code objects `make` builds (colvars-finder_amd/csrc/build/*.o), read with the LLVM tools of
the ROCm install.  Shared by the CPU tests that check register budgets and kernel-instance coverage."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "colvars-finder_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"


def built_objects():
    """Runs `make` and returns the directory of the object files (skips when the LLVM tools are missing)."""
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not in this image")
    return os.path.join(CSRC, "build")


def kernels_of(obj, tmp_path):
    """{mangled kernel name: {vgpr_count, private_segment_fixed_size, ...}} of the gfx950 code object inside a host object file."""
    fat, co = str(tmp_path / "x.fatbin"), str(tmp_path / "x.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name is None:
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
    return out


def template_args(name, family):
    """Integer / bool template arguments of an instance of the kernel template `family` from its mangled name
    (`...17ef16_front_kernelILi20ELi3ELi6ELb1EEE...` -> (20, 3, 6, 1)), or None for another kernel."""
    m = re.search(rf"\d+{family}I((?:L[ib]\d+E)+)E", name)
    if m is None:
        return None
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))
