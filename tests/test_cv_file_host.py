"""CPU: the CV model file (export.save_cv_file; include/cvf.h: cvf_cv_file_*): round trip against the layer's tables and
core._CVModel._nets_plan bit for bit, the parser's refusals through ctypes, and the same parser as a stand-alone program under
the address and undefined-behaviour sanitizers (csrc/cvf_cv_file.hpp; cases: tests/cv_frame_cases.py)."""
import os
import shutil
import subprocess

import pytest
import torch

from tests import codeobj
from tests import cv_frame_cases as F


@pytest.fixture(scope="module")
def hip():
    from colvarsfinder import _hip
    _hip.lib()
    return _hip


def models():
    """{id: colvar_model()-shaped _CVModel on the CPU}"""
    from colvarsfinder import core, nn
    torch.manual_seed(5)
    mixed, _, _ = F.hip_layer("mixed10")
    weighted, _, _ = F.hip_layer("weighted12_mixed-angle")
    dih, _, _ = F.hip_layer("dih10")
    ae = nn.AutoEncoder([mixed.d_r, 16, 2], [2, 16, mixed.d_r])
    return {"ef": core._CVModel(mixed, nn.EigenFunctions([mixed.d_r, 20, 20, 1], 3)),
            "shared-ef": core._CVModel(weighted, nn.SharedEigenFunctions([weighted.d_r, 12], [12, 6, 1], 2)),
            "ae-encoder": core._CVModel(mixed, ae.encoder),
            "features-only": core._CVModel(dih, nn.EigenFunctions([dih.d_r, 8, 1], 2)),
            "identity": core._CVModel(torch.nn.Identity(), nn.EigenFunctions([2, 20, 20, 1], 2))}


@pytest.fixture(scope="module")
def blobs(hip):
    from colvarsfinder import export
    return {name: export.cv_file_bytes(cv) for name, cv in models().items()}


@pytest.mark.parametrize("name", ["ef", "shared-ef", "ae-encoder", "features-only", "identity"])
def test_round_trip_bit_for_bit(hip, tmp_path, name):
    from colvarsfinder import core, export, pp
    cv = models()[name]
    path = export.save_cv_file(cv, str(tmp_path / "cv.cvf"))
    blob = open(path, "rb").read()
    assert blob == export.cv_file_bytes(cv)
    got = F.read_cv_file(blob)
    layer, nets = cv._pp_and_nets()
    d, upto, k, params = core._CVModel._nets_plan(nets)
    assert bytes(d) == blob[F.MLP_OFFSET:F.PP_OFFSET]                                  # every cvf_mlp_desc field
    assert (got["upto_layer"], got["k"]) == (upto, k)
    assert got["mlp"]["n_params"] == d.n_params and got["mlp"]["dims"][:upto + 1] == list(d.dims)[:upto + 1]
    theta = torch.cat([p.detach().reshape(-1) for p in params]).numpy()
    assert got["tables"]["theta"].tobytes() == theta.astype("<f4").tobytes()
    T, S = got["tables"], got["pp"]
    if isinstance(layer, torch.nn.Identity):
        assert S == dict(zip(F.PP_SCALARS, (hip.PP_IDENTITY, 2, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0)))
        assert all(T[n].size == 0 for n in T if n != "theta")
        return
    assert isinstance(layer, pp.AlignFeatureLayer)
    want = dict(mode=hip.PP_ALIGN if layer.aligned else hip.PP_FEATURES, n_coord=3 * layer.n_atoms, n_align=layer.align_idx.numel(),
                n_rec=layer.rec.shape[0], d_r=layer.d_r, use_angle_value=int(layer.use_angle_value),
                has_position=int((layer.rec[:, 0] == hip.FEAT_POSITION).any()), flags=layer._flags, n_slot=layer._n_slot,
                n_rec_slot=layer._n_rec_slot, n_mrec=layer.mrec.shape[0], n_ref=layer._n_ref)
    assert S == want
    for tname in ("align_idx", "ref_c", "rec", "atom_align", "atom_slot", "rec_slot", "slot_atom", "mrec", "slot_row"):
        ref = getattr(layer, tname).numpy().reshape(-1)
        assert T[tname].tobytes() == ref.tobytes() and T[tname].dtype.kind == ref.dtype.kind, tname
    if layer.align_w is None:
        assert T["align_w"].size == 0
    else:
        assert T["align_w"].tobytes() == layer.align_w.numpy().tobytes()
    assert all(off % 16 == 0 for off, n in got["offsets"].values() if n)


def test_models_the_nets_plan_rejects_raise_with_its_reason(hip):
    from colvarsfinder import core, export, nn
    from tests.foreign_modules import PairDistances
    layer, _, _ = F.hip_layer("mixed10")
    reg = nn.RegAutoEncoder([layer.d_r, 16, 3], [3, 16, layer.d_r], [3, 12, 1], 2)
    with pytest.raises(NotImplementedError, match="RegModel"):
        export.save_cv_file(core._CVModel(layer, nn.RegModel(reg, [0, 1])), "/dev/null")
    with pytest.raises(NotImplementedError, match="PairDistances"):
        export.save_cv_file(core._CVModel(PairDistances(6), nn.EigenFunctions([15, 8, 1], 2)), "/dev/null")
    with pytest.raises(NotImplementedError, match="colvar_model"):
        export.save_cv_file(torch.nn.Linear(3, 1), "/dev/null")


def bad_blobs(blobs):
    """{id: (blob, words the message must contain)} - every one must be refused."""
    good = blobs["ef"]
    info = F.read_cv_file(good)
    N = info["pp"]["n_coord"] // 3
    out = {}
    cuts = {1: "magic", F.DIR_OFFSET - 1: "header", F.DIR_OFFSET: "directory", F.DIR_OFFSET + 24 * len(F.TABLE_IDS) - 1: "directory"}
    for name, (off, n) in info["offsets"].items():
        if n:
            cuts[off] = "past the end"                   # the file ends where this table begins
            cuts[off + 4 * n - 1] = "past the end"       # ... and one byte short of its end
    for cut, words in cuts.items():
        if cut < len(good):
            out[f"cut-{cut}"] = (good[:cut], words)
    out["magic"] = (b"CVF2" + good[4:], "magic")
    out["version"] = (F.patched(good, 4, "<i", 2), "version")
    out["max-nets"] = (F.patched(good, 8, "<i", 16), "CVF_MAX_NETS")
    e = F.dir_entry_offset("rec")
    out["offset-past-end"] = (F.patched(good, e + 16, "<q", (len(good) + 15) // 16 * 16), "rec")
    out["offset-huge"] = (F.patched(good, e + 16, "<q", 2 ** 62), "rec")
    out["count-vs-n_rec"] = (F.patched(good, e + 8, "<q", info["offsets"]["rec"][1] - 6), "n_rec")
    out["count-negative"] = (F.patched(good, F.dir_entry_offset("theta") + 8, "<q", -4), "theta")
    out["table-id"] = (F.patched(good, e, "<i", 12), "table id")
    out["table-twice"] = (F.patched(good, e, "<i", F.TABLE_IDS["ref_c"]), "twice")
    rec_off = info["offsets"]["rec"][0]
    out["atom-equal-N"] = (F.patched(good, rec_off + 4, "<i", N), "atom")
    out["rec-type"] = (F.patched(good, rec_off, "<i", 4), "type")
    out["out-past-d_r"] = (F.patched(good, rec_off + 20, "<i", info["pp"]["d_r"]), "output")
    out["align-idx-N"] = (F.patched(good, info["offsets"]["align_idx"][0], "<i", N), "align_idx")
    out["slot-atom-N"] = (F.patched(good, info["offsets"]["slot_atom"][0], "<i", N), "slot_atom")
    L1 = F.MAX_LAYERS + 1
    w_off0 = F.MLP_OFFSET + 4 * (2 + L1 + F.MAX_LAYERS)
    out["w_off-past-theta"] = (F.patched(good, w_off0, "<i", info["mlp"]["n_params"] - 3), "w_off")
    out["b_off-negative"] = (F.patched(good, w_off0 + 4 * F.MAX_NETS * F.MAX_LAYERS, "<i", -1), "b_off")
    out["act-code"] = (F.patched(good, F.MLP_OFFSET + 4 * (2 + L1), "<i", 7), "act")
    out["n_layers"] = (F.patched(good, F.MLP_OFFSET + 4, "<i", 13), "n_layers")
    out["mode-factored"] = (F.patched(good, F.PP_OFFSET, "<i", 2), "mode")
    out["n_coord"] = (F.patched(good, F.PP_OFFSET + 4, "<i", info["pp"]["n_coord"] + 1), "n_coord")
    out["k"] = (F.patched(good, F.TAIL_OFFSET + 4, "<i", 2), "k = 2")
    return out


def test_parser_accepts_good_blobs_and_refuses_bad_ones(hip, blobs):
    lib = hip.lib()
    for name, blob in blobs.items():
        need = lib.cvf_cv_file_device_bytes(blob, len(blob))
        info = F.read_cv_file(blob)
        end = max(off + 4 * n for off, n in info["offsets"].values())
        start = min(off for off, n in info["offsets"].values() if n)
        assert need == (end - start + 15) // 16 * 16 > 0, (name, lib.cvf_last_error().decode())
    bad = bad_blobs(blobs)
    assert len(bad) > 30
    for name, (blob, words) in bad.items():
        rc = lib.cvf_cv_file_device_bytes(blob, len(blob))
        why = lib.cvf_last_error().decode()
        assert rc < 0, (name, rc)
        assert words in why, (name, why)
    assert lib.cvf_cv_file_device_bytes(None, 0) < 0


def test_parser_under_the_sanitizers(hip, blobs, tmp_path):
    """The parser as a stand-alone program (its own main, no GPU, nothing preloaded), address + undefined-behaviour sanitizers."""
    clang = os.path.join(codeobj.LLVM, "clang++")
    cxx = clang if os.path.exists(clang) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler in this image")
    exe = str(tmp_path / "cv_file_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(codeobj.ROOT, "include"), "-I", codeobj.CSRC, os.path.join(codeobj.ROOT, "tests", "cv_file_check_main.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and cxx == clang and shutil.which("g++"):
        built = subprocess.run([shutil.which("g++")] + cmd[1:], capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "sanitizer" in built.stderr.lower() or "ubsan" in built.stderr:
            pytest.skip("the sanitizer runtime is not in this image: " + built.stderr.strip().splitlines()[-1])
        raise AssertionError(built.stderr)
    files, want = [], []
    for name, blob in list(blobs.items()) + [(n, b) for n, (b, _) in bad_blobs(blobs).items()]:
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
        rc, nbytes = int(line.split()[0]), int(line.split()[1])
        assert (rc == 0) == good, (path, line)
        blob = open(path, "rb").read()
        assert (nbytes if good else rc) == lib.cvf_cv_file_device_bytes(blob, len(blob)), (path, line)   # one parser, two builds
