"""CPU: the one-launch CV evaluation's predicate, symbols, register budget and the conditioning of its accuracy cases
(csrc/cv_frame.hip; cases and mirrors: tests/cv_frame_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import cv_frame_cases as F

NEW = ("cvf_cv_frame_supported", "cvf_cv_frame_eval", "cvf_cv_file_device_bytes", "cvf_cv_file_bind")


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


@pytest.mark.parametrize("row", F.predicate_table(), ids=lambda r: r[0])
def test_predicate_table(hip, row):
    _, m, upto, pp, want, words = row
    got = hip.lib().cvf_cv_frame_supported(m, upto, pp)
    why = hip.lib().cvf_last_error().decode()
    assert got == want, why
    if want == 0:
        assert words in why, why
        assert "three-call recipe" in why and "cvf_cv_nets_eval" in why, why   # the refusal names the route that takes the shape


def test_lds_total_is_the_mirror_and_the_64_kib_edge(hip):
    """The predicate's LDS total against its Python mirror on either side of 64 KiB: k = 8 identity chains of seven hidden layers, the width
    stepped until the total passes the limit."""
    lib = hip.lib()
    seen = set()
    for w in range(200, 257):
        m, pp = F.mlp([512] + [w] * 7 + [1], 8), F.pp_desc(hip.PP_IDENTITY, 512, 512)
        fits = 4 * F.lds_floats(m, 8, pp) <= 64 * 1024
        assert lib.cvf_cv_frame_supported(m, 8, pp) == int(fits), (w, lib.cvf_last_error().decode())
        seen.add(fits)
    assert seen == {True, False}


def test_the_large_lds_case_sits_between_48_and_64_kib(hip):
    """A-lds-over-48k on mixed10 needs the launch's dynamic-LDS limit raised: the case must stay on that path and be accepted."""
    layer, _, _ = F.hip_layer("mixed10")
    m, upto, k, _ = F.plan_of(F.nets_for("mixed10", "A-lds-over-48k"))
    pp = F.pp_desc(hip.PP_ALIGN, 3 * layer.n_atoms, layer.d_r, n_rec=layer.rec.shape[0], n_align=layer.align_idx.numel())
    assert 48 * 1024 < 4 * F.lds_floats(m, upto, pp) <= 64 * 1024
    assert hip.lib().cvf_cv_frame_supported(m, upto, pp) == 1, hip.lib().cvf_last_error().decode()


def test_symbols_declared_bound_and_defined(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert set(hip._SIGNATURES) == declared
    assert ctypes.sizeof(hip.CVModel) == ctypes.sizeof(hip.MLPDesc) + ctypes.sizeof(hip.PPDesc) + 16


def test_kernel_resources(tmp_path):
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "cv_frame.o"), tmp_path)
    assert kernels and any("cv_frame_kernel" in n for n in kernels)
    for name, r in kernels.items():
        assert r["vgpr_count"] <= 128, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


@pytest.mark.parametrize("lid,nid", F.ACCURACY, ids=lambda v: v)
def test_accuracy_cases_are_well_conditioned(lid, nid):
    """A condition, not a measurement: the fp32 CPU evaluation of every accuracy case lies within COND_TOL of the fp64 one, so
    that what the GPU test measures is the kernels' arithmetic and not the case's conditioning."""
    from tests.test_cv_jacobian_gpu import rel_err
    _, traj, _ = F.hip_layer(lid)
    nets = F.nets_for(lid, nid)
    xi64, J64 = F.cpu_eval(lid, nets, traj, torch.float64)
    xi32, J32 = F.cpu_eval(lid, nets, traj, torch.float32)
    ej, ex = rel_err(J32, J64), rel_err(xi32, xi64)
    print(f"[cvframe] conditioning {lid} {nid}: J {ej:.2e} xi {ex:.2e}")
    assert np.isfinite(J64).all() and ej <= F.COND_TOL and ex <= F.COND_TOL
