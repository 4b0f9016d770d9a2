"""CPU: form C of the CV evaluation kernels (k scalar chains on one trunk) - the predicates of the three
routes, the Python mirrors of their LDS and scratch totals, the plan core._CVModel._nets_plan_shared builds, the form-C model
file through ctypes and as a stand-alone program under the host sanitizers, and the conditioning of every accuracy case of
tests/test_cv_shared_gpu.py (cases: tests/cv_shared_cases.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import cv_frame_cases as F
from tests import cv_frame_large_cases as G
from tests import cv_shared_cases as S

NEW = ["cvf_cv_nets_shared_supported", "cvf_cv_nets_shared_scratch_floats", "cvf_cv_nets_shared_eval", "cvf_cv_frame_shared_supported",
       "cvf_cv_frame_shared_eval", "cvf_cv_frame_large_shared_supported", "cvf_cv_frame_large_shared_lds_bytes",
       "cvf_cv_frame_large_shared_eval", "cvf_cv_file_n_shared"]


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def test_symbols_declared_bound_and_defined(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert ctypes.sizeof(hip.CVModel) == ctypes.sizeof(hip.MLPDesc) + ctypes.sizeof(hip.PPDesc) + 16   # cvf_cv_model keeps its size


# ------------------------------------------------------------------------------------------------ predicates
def predicates(hip, m, ns, pp_wave, pp_large):
    """[(name, answer, reason)] of the three routes' predicates."""
    lib = hip.lib()
    out = []
    for name, fn, args in (("nets", lib.cvf_cv_nets_shared_supported, (m, ns, 1)),
                           ("frame", lib.cvf_cv_frame_shared_supported, (m, ns, pp_wave)),
                           ("frame-large", lib.cvf_cv_frame_large_shared_supported, (m, ns, pp_large))):
        got = fn(*args)
        out.append((name, got, lib.cvf_last_error().decode()))
    return out


def test_n_shared_out_of_range_and_broken_aliases_are_refused(hip):
    A = hip.PP_ALIGN
    m, ns = S.shared_mlp([30, 20, 20], [20, 1], 3)
    ppw, ppl = F.pp_desc(A, 30, 30), G.pp_large(A, 195, 30)
    plain = {"nets": "cvf_cv_nets_eval", "frame": "cvf_cv_frame_eval", "frame-large": "cvf_cv_frame_large_eval"}
    for name, got, why in predicates(hip, m, ns, ppw, ppl):
        assert got == 1, (name, why)
    for name, got, why in predicates(hip, m, 0, ppw, ppl):
        assert got == 0 and "n_shared = 0" in why and plain[name] in why, (name, why)   # names the existing entry point
    for bad in (m.n_layers, m.n_layers + 1, -1):
        for name, got, why in predicates(hip, m, bad, ppw, ppl):
            assert got == 0 and f"n_shared = {bad}" in why, (name, why)
    for name, got, why in predicates(hip, m, 1, ppw, ppl):   # fewer shared layers than aliased: legal (the offsets need not differ)
        assert got == 1, (name, why)
    for field in ("w_off", "b_off"):
        b, _ = S.shared_mlp([30, 20, 20], [20, 1], 3)
        getattr(b, field)[2][1] += 1
        for name, got, why in predicates(hip, b, ns, ppw, ppl):
            assert got == 0 and "net 2" in why and "layer 1" in why and field in why, (name, why)
    plain_ef = F.mlp([30, 20, 20, 1], 3)   # three unshared chains: refused under any n_shared > 0
    for name, got, why in predicates(hip, plain_ef, 1, ppw, ppl):
        assert got == 0 and "net 1" in why and "layer 0" in why, (name, why)
    vec, _ = S.shared_mlp([30, 20], [20, 2], 3)
    for name, got, why in predicates(hip, vec, 1, ppw, ppl):
        assert got == 0 and "scalar" in why, (name, why)
    nine, _ = S.shared_mlp([30, 20], [20, 1], 8)
    nine.n_nets = 9
    for name, got, why in predicates(hip, nine, 1, ppw, ppl):
        assert got == 0 and "9 nets" in why, (name, why)
    lib = hip.lib()
    assert lib.cvf_cv_nets_shared_scratch_floats(m, 0, 64, 1) == 0 and lib.cvf_cv_nets_shared_scratch_floats(b, ns, 64, 1) == 0
    assert lib.cvf_cv_frame_large_shared_lds_bytes(m, 0, ppl, None) < 0
    # the limits of the namesakes still hold, with their words
    wide, _ = S.shared_mlp([30, 257], [257, 1], 3)
    assert lib.cvf_cv_frame_shared_supported(wide, 1, ppw) == 0 and "257 wide" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_frame_large_shared_supported(wide, 1, ppl) == 0 and "257 wide" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_nets_shared_supported(wide, 1, 1) == 1
    assert lib.cvf_cv_frame_shared_supported(m, ns, F.pp_desc(A, 195, 30)) == 0 and "n_coord = 195" in lib.cvf_last_error().decode()


def test_one_trunk_fits_where_eight_copies_do_not(hip):
    """The `lds-over` case of tests/cv_frame_cases.py - eight heads [256, 1] on a trunk [30] + [256] * 11: cvf_cv_frame_supported
    refuses its k-fold activations (the aliased description and the unshared one alike), cvf_cv_frame_shared_supported accepts the
    one trunk."""
    lib, pp = hip.lib(), F.pp_desc(hip.PP_ALIGN, 30, 30)
    m, ns = S.shared_mlp([30] + [256] * 11, [256, 1], 8)
    assert ns == 11 and m.n_layers == 12
    assert lib.cvf_cv_frame_supported(m, 12, pp) == 0 and "bytes of LDS" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_frame_supported(F.mlp([30] + [256] * 11 + [1], 8), 12, pp) == 0
    assert lib.cvf_cv_frame_shared_supported(m, ns, pp) == 1, lib.cvf_last_error().decode()
    assert 4 * S.lds_floats(m, ns, pp) <= 64 * 1024 < 4 * F.lds_floats(m, 12, pp)


def test_lds_totals_are_the_mirrors(hip):
    """Wave kernel: the mirror on either side of 64 KiB (k = 8 heads of seven layers on an identity trunk of four, all w wide, w
    stepped); workgroup kernel: bytes and rows_per_pass of the mirror, on shapes whose row table fits whole and in part."""
    lib = hip.lib()
    seen = set()
    for w in range(140, 200):
        m, ns = S.shared_mlp([512] + [w] * 4, [w] * 7 + [1], 8)
        pp = F.pp_desc(hip.PP_IDENTITY, 512, 512)
        fits = 4 * S.lds_floats(m, ns, pp) <= 64 * 1024
        assert lib.cvf_cv_frame_shared_supported(m, ns, pp) == int(fits), (w, lib.cvf_last_error().decode())
        seen.add(fits)
    assert seen == {True, False}
    rows = ctypes.c_int32(-1)
    for trunk, head, k, n_ref in (([66, 20, 20], [20, 1], 3, 16), ([66, 20, 20], [20, 1], 8, 1840), ([384, 20, 20], [20, 1], 6, 608),
                                  ([512] + [256] * 10, [256, 256, 1], 8, 6144), ([30, 256], [256, 1], 8, 6144)):
        m, ns = S.shared_mlp(trunk, head, k)
        pp = G.pp_large(hip.PP_ALIGN, 15000, trunk[0], n_ref=n_ref)
        want, rpp = S.large_lds_layout(m, ns, pp)
        got = lib.cvf_cv_frame_large_shared_lds_bytes(m, ns, pp, ctypes.byref(rows))
        assert want is not None and got == want and rows.value == rpp, (trunk, head, k, n_ref, got, want, rows.value, rpp)
    assert rpp < 8   # the last shape walks its eight cotangent rows in more than one pass


def test_scratch_formula_counts_the_trunk_once(hip):
    lib = hip.lib()
    for trunk, head, k in (([30, 20, 20], [20, 1], 3), ([30, 12], [12, 6, 1], 2), ([7, 10, 10, 10], [10, 1], 2), ([30, 256, 256], [256, 1], 8),
                           ([30, 20, 20], [20, 1], 1)):
        m, ns = S.shared_mlp(trunk, head, k)
        for B in (1, 64, 65, 1000):
            for want_g in (0, 1):
                assert lib.cvf_cv_nets_shared_scratch_floats(m, ns, B, want_g) == S.scratch_floats(m, ns, B, bool(want_g)), (trunk, k, B, want_g)
            if k > 1:
                assert lib.cvf_cv_nets_shared_scratch_floats(m, ns, B, 1) < lib.cvf_cv_nets_scratch_floats(m, m.n_layers, B, 1)
        assert lib.cvf_cv_nets_shared_scratch_floats(m, ns, 0, 1) == 0


# ------------------------------------------------------------------------------------------------ the plan
def reg_cv(layer, K=2, shared=True):
    from colvarsfinder import core
    cv = core._CVModel(layer, S.build_nets("C-reg", layer.d_r) if K == 2 else reg_model_k3(layer.d_r))
    cv.shared_trunk = shared
    return cv


def reg_model_k3(d_r):
    from colvarsfinder import nn
    torch.manual_seed(33)
    return nn.RegModel(nn.RegAutoEncoder([d_r, 16, 3], [3, 16, d_r], [3, 12, 1], 3), S.REG_CVEC[3])


def test_plan_lists_every_tensor_once(hip):
    from colvarsfinder import core
    ef = S.build_nets("C-head2", 30)
    d, L, k, params, ns = core._CVModel._nets_plan_shared(ef)
    assert (L, k, ns) == (3, 2, 1) and len(params) == len({id(p) for p in params}) == 2 + 2 * 4
    assert d.n_params == sum(p.numel() for p in ef.parameters()) == 31 * 12 + 2 * (13 * 6 + 7)
    assert [d.w_off[i][0] for i in range(2)] == [0, 0] and d.w_off[0][1] != d.w_off[1][1]
    d4, L4, k4, params4 = core._CVModel._nets_plan(ef)   # (form A: the trunk's tensors once per chain)
    assert d4.n_params == 2 * (31 * 12 + 13 * 6 + 7) and list(d4.dims) == list(d.dims) and list(d4.act) == list(d.act)
    # a RegModel: the chains in cvec order, no activation at the boundary, boundary width 3
    reg = S.build_nets("C-reg", 30)
    d, L, k, params, ns = core._CVModel._nets_plan_shared(reg)
    assert (L, k, ns) == (4, 2, 2) and list(d.dims)[:5] == [30, 16, 3, 12, 1] and list(d.act)[:4] == [1, 0, 1, 0]
    enc = [p for p in reg.encoder.parameters()]
    assert [id(p) for p in params[:4]] == [id(p) for p in enc]
    assert [id(p) for p in params[4:8]] == [id(p) for p in reg.reg[1].parameters()]      # cvec = [1, 0]: head 0 is reg[1]
    assert [id(p) for p in params[8:]] == [id(p) for p in reg.reg[0].parameters()]
    assert d.n_params == sum(p.numel() for p in params) == 31 * 16 + 17 * 3 + 2 * (4 * 12 + 13)


def test_plan_refusals_carry_the_reason(hip):
    from colvarsfinder import core, nn
    plan = core._CVModel._nets_plan_shared
    with pytest.raises(TypeError, match="EigenFunctions"):
        plan(nn.EigenFunctions([30, 8, 1], 2))
    rae = nn.RegAutoEncoder([30, 16, 3], [3, 16, 30], [3, 12, 1], 2)
    rae.reg[1] = nn.create_sequential_nn([3, 11, 1])
    with pytest.raises(TypeError, match="differ in architecture"):
        plan(nn.RegModel(rae, [0, 1]))
    rae = nn.RegAutoEncoder([30, 16, 3], [3, 16, 30], [3, 12, 1], 2)
    rae.reg[0] = torch.nn.Sequential(torch.nn.Linear(3, 12), torch.nn.Dropout(), torch.nn.Linear(12, 1))
    with pytest.raises(TypeError, match="Dropout"):
        plan(nn.RegModel(rae, [0, 1]))
    with pytest.raises(TypeError, match="GELU"):
        plan(nn.SharedEigenFunctions([30, 8], [8, 1], 2, activation=torch.nn.GELU()))
    with pytest.raises(TypeError, match="k = 9"):
        plan(nn.SharedEigenFunctions([30, 8], [8, 1], 9))


def test_the_option_is_opt_in(hip):
    from colvarsfinder import core, export, nn
    layer, _, _ = F.hip_layer("mixed10")
    cv = reg_cv(layer, shared=False)
    assert core._CVModel.shared_trunk is False and cv.shared_trunk is False
    kind, why = cv.nets_route()
    assert kind == "torch" and "RegModel" in why and "shared_trunk" in why
    with pytest.raises(NotImplementedError, match="RegModel.*shared_trunk"):
        export.cv_file_bytes(cv)
    cv.shared_trunk = True
    assert cv.nets_route() == ("hip", None)
    sef = core._CVModel(layer, S.build_nets("C-head2", layer.d_r))
    plain = export.cv_file_bytes(sef)
    assert sef.nets_route() == ("hip", None) and S.file_n_shared(plain) == 0
    sef.shared_trunk = True
    assert sef.nets_route() == ("hip", None) and S.file_n_shared(export.cv_file_bytes(sef)) == 1
    sef.shared_trunk = False
    assert export.cv_file_bytes(sef) == plain                                  # with False the bytes are today's:
    _, sef_nets = sef._pp_and_nets()                                           # core._CVModel._nets_plan's description and theta
    d_a, _, _, params_a = core._CVModel._nets_plan(sef_nets)                   # (the trunk once per chain), n_shared 0
    got = F.read_cv_file(plain)
    assert bytes(d_a) == plain[F.MLP_OFFSET:F.PP_OFFSET]
    assert got["tables"]["theta"].tobytes() == torch.cat([p.detach().reshape(-1) for p in params_a]).numpy().astype("<f4").tobytes()
    assert got["mlp"]["n_params"] == 2 * ((layer.d_r + 1) * 12 + 13 * 6 + 7) and S.file_n_shared(plain) == 0
    other = core._CVModel(layer, nn.EigenFunctions([layer.d_r, 8, 1], 2))      # models of the other types: as with False
    before = export.cv_file_bytes(other)
    other.shared_trunk = True
    assert export.cv_file_bytes(other) == before and other.nets_route() == ("hip", None)


# ------------------------------------------------------------------------------------------------ the file
def file_models():
    """{id: (cv with shared_trunk = True, expected n_shared)}"""
    from colvarsfinder import core
    mixed, _, _ = F.hip_layer("mixed10")
    weighted, _, _ = F.hip_layer("weighted12_mixed-angle")
    sef = core._CVModel(weighted, S.build_nets("C-head2", weighted.d_r))
    sef.shared_trunk = True
    ident = core._CVModel(torch.nn.Identity(), S.build_nets("C-k3", 2))
    ident.shared_trunk = True
    return {"shared-ef": (sef, 1), "reg": (reg_cv(mixed), 2), "reg-k3": (reg_cv(mixed, K=3), 2), "identity": (ident, 2)}


@pytest.fixture(scope="module")
def blobs(hip):
    from colvarsfinder import export
    return {name: export.cv_file_bytes(cv) for name, (cv, _) in file_models().items()}


def bad_blobs(hip, blobs):
    """{id: (blob, words the message must contain)} - every one must be refused."""
    from colvarsfinder import core, export, nn
    at = F.TAIL_OFFSET + 12
    good = blobs["reg"]
    n_layers = S.read_cv_file(good)["mlp"]["n_layers"]
    mixed, _, _ = F.hip_layer("mixed10")
    torch.manual_seed(5)
    ef = export.cv_file_bytes(core._CVModel(mixed, nn.EigenFunctions([mixed.d_r, 20, 20, 1], 3)))   # the unshared blob
    L1 = F.MAX_LAYERS + 1
    w_off = lambda i, l: F.MLP_OFFSET + 4 * (2 + L1 + F.MAX_LAYERS + i * F.MAX_LAYERS + l)
    w11 = S.read_cv_file(good)["mlp"]["w_off"][1][1]
    return {"n_shared-n_layers": (F.patched(good, at, "<i", n_layers), "n_shared"),
            "n_shared-minus-1": (F.patched(good, at, "<i", -1), "n_shared"),
            "n_shared-on-unshared": (F.patched(ef, at, "<i", 1), "net 1 does not share layer 0"),
            "alias-broken": (F.patched(good, w_off(1, 1), "<i", w11 + 1), "net 1 does not share layer 1"),
            "upto-cut": (F.patched(good, F.TAIL_OFFSET, "<i", n_layers - 1), "upto_layer")}


@pytest.mark.parametrize("name", ["shared-ef", "reg", "reg-k3", "identity"])
def test_file_round_trip(hip, name):
    from colvarsfinder import core, export
    cv, ns = file_models()[name]
    blob = export.cv_file_bytes(cv)
    got = S.read_cv_file(blob)
    _, nets = cv._pp_and_nets()
    d, L, k, params, ns_plan = core._CVModel._nets_plan_shared(nets)
    assert got["n_shared"] == ns == ns_plan and (got["upto_layer"], got["k"]) == (L, k)
    assert bytes(d) == blob[F.MLP_OFFSET:F.PP_OFFSET]
    theta = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    assert got["tables"]["theta"].tobytes() == theta.astype("<f4").tobytes()              # the trunk once
    assert got["mlp"]["n_params"] == theta.size == sum(p.numel() for p in nets.parameters())   # (parameters() yields shared tensors once)
    for i in range(k):
        for l in range(ns):
            assert got["mlp"]["w_off"][i][l] == got["mlp"]["w_off"][0][l] and got["mlp"]["b_off"][i][l] == got["mlp"]["b_off"][0][l]
    lib = hip.lib()
    assert lib.cvf_cv_file_device_bytes(blob, len(blob)) > 0, lib.cvf_last_error().decode()
    assert lib.cvf_cv_file_n_shared(blob, len(blob)) == ns


def test_file_refusals_and_old_files(hip, blobs):
    from colvarsfinder import core, export, nn
    lib = hip.lib()
    for name, (blob, words) in bad_blobs(hip, blobs).items():
        rc = lib.cvf_cv_file_device_bytes(blob, len(blob))
        why = lib.cvf_last_error().decode()
        assert rc < 0 and words in why, (name, rc, why)
        assert lib.cvf_cv_file_n_shared(blob, len(blob)) == rc, name
    layer, _, _ = F.hip_layer("mixed10")
    old = export.cv_file_bytes(core._CVModel(layer, nn.EigenFunctions([layer.d_r, 8, 1], 2)))
    assert lib.cvf_cv_file_n_shared(old, len(old)) == 0 and S.file_n_shared(old) == 0
    assert lib.cvf_cv_file_n_shared(old[:100], 100) < 0 and lib.cvf_cv_file_n_shared(None, 0) < 0


def test_parser_under_the_sanitizers(hip, blobs, tmp_path):
    """tests/cv_shared_file_check_main.cpp - the parser with the n_shared field as a stand-alone program (its own main, no GPU,
    nothing preloaded) under the address and undefined-behaviour sanitizers, as tests/test_cv_file_host.py builds its sibling."""
    clang = os.path.join(codeobj.LLVM, "clang++")
    cxx = clang if os.path.exists(clang) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler in this image")
    exe = str(tmp_path / "cv_shared_file_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(codeobj.ROOT, "include"), "-I", codeobj.CSRC,
           os.path.join(codeobj.ROOT, "tests", "cv_shared_file_check_main.cpp"), "-o", exe]
    # is the sanitizer runtime here at all?  Asked with an empty program, so that no error in the real source can pass for its absence
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = subprocess.run([cxx] + flags + [str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    if probe.returncode != 0 and cxx == clang and shutil.which("g++"):
        cxx = shutil.which("g++")
        probe = subprocess.run([cxx] + flags + [str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no host compiler here links the sanitizer runtime: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    built = subprocess.run([cxx] + cmd[1:], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    files, want = [], []
    bad = bad_blobs(hip, blobs)
    cut = {f"cut-{n}": (blobs["reg"][:n], "") for n in (F.TAIL_OFFSET + 12, F.TAIL_OFFSET + 15, F.DIR_OFFSET)}
    for name, blob in list(blobs.items()) + [(n, b) for n, (b, _) in list(bad.items()) + list(cut.items())]:
        p = tmp_path / f"{name}.cvf"
        p.write_bytes(blob)
        files.append(str(p))
        want.append(name in blobs)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(files)
    lib = hip.lib()
    for path, good, line in zip(files, want, lines):
        rc, nbytes, ns = (int(v) for v in line.split()[:3])
        blob = open(path, "rb").read()
        assert (rc == 0) == good, (path, line)
        assert (nbytes if good else rc) == lib.cvf_cv_file_device_bytes(blob, len(blob)), (path, line)   # one parser, two builds
        assert (ns if good else rc) == lib.cvf_cv_file_n_shared(blob, len(blob)), (path, line)


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("lid,nid", S.ACCURACY + [c for c in S.COEF if c not in S.ACCURACY] + S.LARGE_ACCURACY
                         + [c for c in S.LARGE_COEF if c not in S.LARGE_ACCURACY], ids=lambda v: v)
def test_accuracy_cases_are_well_conditioned(lid, nid):
    """A condition, not a measurement: the fp32 CPU evaluation of every accuracy case lies within COND_TOL of the fp64 one, so
    that what the GPU test measures is the kernels' arithmetic and not the case's conditioning."""
    from tests.test_cv_jacobian_gpu import rel_err
    traj = S.frames(lid)
    nets = S.nets_for(lid, nid)
    xi64, J64 = S.cpu_eval(lid, nets, traj, torch.float64)
    xi32, J32 = S.cpu_eval(lid, nets, traj, torch.float32)
    ej, ex = rel_err(J32, J64), rel_err(xi32, xi64)
    print(f"[cvshared] conditioning {lid} {nid}: J {ej:.2e} xi {ex:.2e}")
    assert np.isfinite(J64).all() and ej <= S.COND_TOL and ex <= S.COND_TOL


def test_the_trained_reg_model_case_is_well_conditioned():
    """The RegModel K = 3 case of the FrameCV test (cvec = [2, 0, 1]) on mixed10."""
    from tests.test_cv_jacobian_gpu import rel_err
    traj = S.frames("mixed10")
    nets = reg_model_k3(F.d_r_of("mixed10"))
    xi64, J64 = F.cpu_eval("mixed10", nets, traj, torch.float64)
    xi32, J32 = F.cpu_eval("mixed10", nets, traj, torch.float32)
    assert rel_err(J32, J64) <= S.COND_TOL and rel_err(xi32, xi64) <= S.COND_TOL
