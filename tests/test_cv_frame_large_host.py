"""CPU: the workgroup-per-frame CV evaluation's predicate, LDS layout, symbols, register budget and the conditioning of its
accuracy cases (csrc/cv_frame_large.hip; cases and mirrors: tests/cv_frame_large_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import cv_frame_cases as F
from tests import cv_frame_large_cases as G

NEW = ("cvf_cv_frame_large_supported", "cvf_cv_frame_large_lds_bytes", "cvf_cv_frame_large_eval")


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def lds_of(hip, m, upto, pp):
    rpp = ctypes.c_int32(-7)
    return hip.lib().cvf_cv_frame_large_lds_bytes(m, upto, pp, ctypes.byref(rpp)), rpp.value


@pytest.mark.parametrize("row", G.predicate_table(), ids=lambda r: r[0])
def test_predicate_table(hip, row):
    _, m, upto, pp, want, words = row
    got = hip.lib().cvf_cv_frame_large_supported(m, upto, pp)
    why = hip.lib().cvf_last_error().decode()
    assert got == want, why
    nbytes, rpp = lds_of(hip, m, upto, pp)
    if want == 0:
        assert words in why, why
        assert "three-call recipe" in why and "cvf_cv_nets_eval" in why, why   # the refusal names the route that takes the shape
        assert nbytes < 0 and rpp == -7
    else:
        assert 0 < nbytes <= G.LDS_LIMIT and rpp >= 1


def test_refusals_have_their_own_words(hip):
    rows = {r[0]: r for r in G.predicate_table()}
    seen = set()
    for name in ("identity", "factored", "no-mrec", "no-atom_align", "no-slot_row", "no-slot_atom", "no-atom_slot"):
        _, m, upto, pp, _, _ = rows[name]
        assert hip.lib().cvf_cv_frame_large_supported(m, upto, pp) == 0
        seen.add(hip.lib().cvf_last_error().decode())
    assert len(seen) == 7, seen


def test_lds_total_is_the_mirror_on_either_side_of_160_kib(hip):
    """k = 8 chains of nine hidden layers over a 6144-row table (72 KiB a row), the width stepped until not even one row fits."""
    seen = set()
    for w in range(200, 257):
        m, pp = F.mlp([512] + [w] * 9 + [1], 8), G.pp_large(hip.PP_ALIGN, 15000, 512, n_ref=6144)
        want, rpp = G.lds_layout(m, 10, pp)
        got, got_rpp = lds_of(hip, m, 10, pp)
        assert hip.lib().cvf_cv_frame_large_supported(m, 10, pp) == int(want is not None), (w, hip.lib().cvf_last_error().decode())
        if want is None:
            assert got < 0 and "bytes of LDS" in hip.lib().cvf_last_error().decode()
        else:
            assert (got, got_rpp) == (want, 1) and got <= G.LDS_LIMIT, w
        seen.add(want is not None)
    assert seen == {True, False}


def test_rows_per_pass_is_the_mirror_where_it_drops_below_k(hip):
    """k = 8 [384, 20, 20, 1] chains, n_ref stepped: all eight rows in one pass, then fewer, down to one."""
    m = F.mlp([384, 20, 20, 1], 8)
    seen = []
    for n_ref in list(range(1500, 1700, 7)) + [2000, 3000, 4000, 6144]:
        pp = G.pp_large(hip.PP_ALIGN, 15000, 384, n_ref=n_ref)
        got = lds_of(hip, m, 3, pp)
        assert got == G.lds_layout(m, 3, pp), n_ref
        assert got[0] <= G.LDS_LIMIT and (got[1] == 8 or got[0] + 12 * n_ref > G.LDS_LIMIT)   # the largest that fits
        seen.append(got[1])
    assert seen[0] == 8 and 7 in seen and seen[-1] == 1 and seen == sorted(seen, reverse=True)
    # form B counts the outputs of the one chain; a NULL rows_per_pass is allowed
    mb, pp = F.mlp([384, 20, 8]), G.pp_large(hip.PP_FEATURES, 900, 384, n_ref=6144)
    assert lds_of(hip, mb, 2, pp) == G.lds_layout(mb, 2, pp) and lds_of(hip, mb, 2, pp)[1] < 8
    assert hip.lib().cvf_cv_frame_large_lds_bytes(mb, 2, pp, None) == G.lds_layout(mb, 2, pp)[0]


@pytest.mark.parametrize("lid,nid", G.LAYER_CASES, ids=lambda v: v)
def test_the_cases_sit_where_their_names_say(hip, lid, nid):
    """Every layer case is accepted with its real tables' sizes; c5 takes the dynamic-LDS attribute path; dih300-rows walks its
    rows in more than one pass; mixed300w strides records, slots and align atoms twice; the wave kernel declines them all."""
    layer = G.hip_layer(lid)
    m, upto, k, _ = F.plan_of(G.nets_for(lid, nid))
    pp = G.pp_large(hip.PP_ALIGN if layer.aligned else hip.PP_FEATURES, 3 * layer.n_atoms, layer.d_r, n_align=layer.align_idx.numel(),
                    n_slot=layer._n_slot, n_ref=layer._n_ref, n_mrec=layer.mrec.shape[0])
    assert hip.lib().cvf_cv_frame_large_supported(m, upto, pp) == 1, hip.lib().cvf_last_error().decode()
    nbytes, rpp = lds_of(hip, m, upto, pp)
    assert (nbytes, rpp) == G.lds_layout(m, upto, pp)
    assert hip.lib().cvf_cv_frame_supported(m, upto, pp) == 0
    if lid == "c5":
        assert nbytes > 48 * 1024 and (k, layer.d_r, rpp) == (6, 384, 6)
    if lid == "dih300-rows":
        assert k == 8 and rpp < k and nbytes > 48 * 1024
    else:
        assert rpp == k
    if lid == "mixed300w":
        assert layer.align_idx.numel() == 257 and layer.align_w is not None and layer.mrec.shape[0] > 256 and layer._n_slot > 256
    if lid == "mixed1000":
        assert layer.align_idx.numel() == 600


def test_symbols_declared_bound_and_defined(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert set(hip._SIGNATURES) == declared
    assert hip._SIGNATURES["cvf_cv_frame_large_eval"] == hip._SIGNATURES["cvf_cv_frame_eval"]


def test_kernel_resources(tmp_path):
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "cv_frame_large.o"), tmp_path)
    assert kernels and any("cv_frame_large_kernel" in n for n in kernels)
    for name, r in kernels.items():
        print(f"[cvframe-large] {name}: {r['vgpr_count']} VGPRs")
        assert r["vgpr_count"] <= 128, (name, r)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)


@pytest.mark.parametrize("lid,nid", G.ACCURACY, ids=lambda v: v)
def test_accuracy_cases_are_well_conditioned(lid, nid):
    """A condition, not a measurement: the fp32 CPU evaluation of every accuracy case lies within COND_TOL of the fp64 one, so
    that what the GPU test measures is the kernel's arithmetic and not the case's conditioning."""
    from tests.test_cv_jacobian_gpu import rel_err
    traj, _ = G.frames(lid)
    nets = G.nets_for(lid, nid)
    xi64, J64 = G.cpu_eval(lid, nets, traj, torch.float64)
    xi32, J32 = G.cpu_eval(lid, nets, traj, torch.float32)
    ej, ex = rel_err(J32, J64), rel_err(xi32, xi64)
    print(f"[cvframe-large] conditioning {lid} {nid}: J {ej:.2e} xi {ex:.2e}")
    assert np.isfinite(J64).all() and ej <= G.COND_TOL and ex <= G.COND_TOL
