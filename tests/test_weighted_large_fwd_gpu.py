"""GPU (-m gpu): per-atom alignment weights on the streaming alignment kernels (csrc/k1_large.hip: the WEIGHTED twins of the
gather, capture and slice kernels) through the C ABI, against ``oracle.pp.AlignFeature(align_weights=...)`` in fp64.

Each case first asserts the kernel family and instance ``cvf_align_feature_route`` names - the function the launch decides by -
and then runs every output flavour the instance takes.  Bars: those of
``test_gpu_parity.py::test_k1_pipelined_kernel_equals_the_slice_kernel_and_the_oracle`` for the same kernels (rtol 2e-5,
atol 3e-6 max|want|): the weighted arithmetic adds one multiply per align atom to an fp64 sum."""
import numpy as np
import pytest
import torch

from tests.test_align_vjp_gpu import random_features
from tests.weighted_large_cases import (NOT_IGNORED, frames, oracle_features, position_bond_features, position_columns,
                                        weighted_layer, weights_for)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 3e-6
FLAVOURS = ("features", "generator", "rows", "both")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _case(name):
    """(n_atoms, B, align, features, route code, flavours)"""
    from colvarsfinder import _hip as H
    if name == "capture65":      # one full group of eight frames plus a ragged one; partial, non-contiguous align set
        n = 65
        align = sorted(np.random.RandomState(n).choice(n, 40, replace=False).tolist())
        return n, 9, align, random_features(n, n), H.K1_ROUTE_CAPTURE, FLAVOURS
    if name == "capture_vec4_256":   # d_r < 272: the slice kernel's reduction scratch does not fit the staging area
        n = 256
        return n, 19, list(range(n)), random_features(n, n, n_pos=30, n_bond=20, n_angle=10, n_dih=10), H.K1_ROUTE_CAPTURE_VEC4, FLAVOURS
    if name == "slice1_256":
        n = 256
        return n, 19, list(range(n)), position_bond_features(n, 96, 12, n), H.K1_ROUTE_SLICE + 1, FLAVOURS
    if name in ("slice2_2100", "slice3_4100", "slice4_6200"):
        n = int(name.split("_")[1])
        return n, 11 if n == 2100 else 9, list(range(n)), position_bond_features(n, 96, 12, n), H.K1_ROUTE_SLICE + int(name[5]), FLAVOURS
    if name in ("gather_contig_2000", "gather_2000"):   # 1700 feature atoms do not fit the capture buffer; row-major output alone
        n = 2000
        align = list(range(n)) if "contig" in name else sorted(np.random.RandomState(n).choice(n, 1500, replace=False).tolist())
        feats = [("position", tuple(sorted(np.random.RandomState(n + 1).choice(n, 1700, replace=False).tolist())))]
        return n, 9, align, feats, H.K1_ROUTE_GATHER_CONTIG if "contig" in name else H.K1_ROUTE_GATHER, ("rows",)
    raise KeyError(name)


def _run(layer, desc, x, B, flavour, dev):
    """Outputs of one cvf_align_feature_fwd call as rows: dict(rows=..., tiled=..., aux=..., slots=...) of what the flavour writes."""
    from colvarsfinder import _hip
    lib, P, st = _hip.lib(), _hip.ptr, _hip.stream()
    T, d_r, nan = _hip.ntiles(B), layer.d_r, float("nan")
    tiled = torch.full((T * d_r * 64,), nan, device=dev)
    rows = torch.full((B * d_r,), nan, device=dev)
    aux = torch.full((T * 18 * 64,), nan, device=dev)
    scratch = _hip.align_scratch(desc, B, dev)
    if scratch is not None:
        scratch.fill_(nan)
    args = dict(features=(P(tiled), None, None, None), generator=(P(tiled), None, P(aux), P(scratch)),
                rows=(None, P(rows), None, None), both=(P(tiled), P(rows), None, None))[flavour]
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, *args, st), "cvf_align_feature_fwd")
    torch.cuda.synchronize()
    out = {}
    if flavour != "rows":
        assert torch.isfinite(tiled).all(), "tiled output not fully written"
        out["tiled"] = tiled.view(T, d_r, 64).permute(0, 2, 1).reshape(T * 64, d_r)[:B].cpu().numpy()
    if flavour in ("rows", "both"):
        out["rows"] = rows.view(B, d_r).cpu().numpy()
    if flavour == "generator":
        assert torch.isfinite(aux).all(), "aux rows not fully written"
        out["aux"] = aux.view(T, 18, 64).permute(0, 2, 1).reshape(T * 64, 18)[:B].double().cpu().numpy()
        if scratch is not None:
            ns3 = 3 * layer._n_slot
            g = T * 8
            out["slots"] = scratch.view(torch.float32)[:g * ns3 * 8].view(g, ns3, 8).permute(0, 2, 1).reshape(g * 8, ns3)[:B].cpu().numpy()
    return out


@pytest.mark.parametrize("name", ["capture65", "capture_vec4_256", "slice1_256", "slice2_2100", "slice3_4100", "slice4_6200",
                                  "gather_contig_2000", "gather_2000"])
def test_weighted_streaming_forward_vs_oracle(dev, name):
    from colvarsfinder import _hip, pp
    n, B, align, feats, code, flavours = _case(name)
    traj, _, ref = frames(n, B, seed=900 + n)
    w = weights_for(n, len(align))
    layer = weighted_layer(n, align, ref, feats, w, dev)
    desc = layer.pp_desc()
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    want = oracle_features(align, ref, feats, w, traj)
    plain = oracle_features(align, ref, feats, None, traj)
    cols = position_columns(feats)
    assert np.abs(want[:, cols] - plain[:, cols]).max() > NOT_IGNORED
    lib = _hip.lib()
    has_scratch = int(lib.cvf_align_feature_scratch_bytes(desc, B) > 0)
    for flavour in flavours:
        tiled, rows, gen = int(flavour != "rows"), int(flavour in ("rows", "both")), int(flavour == "generator")
        assert lib.cvf_align_feature_route(desc, B, tiled, rows, gen, gen * has_scratch) == code, (name, flavour)
        out = _run(layer, desc, x, B, flavour, dev)
        for key in ("tiled", "rows"):
            if key in out:
                err = np.abs(out[key] - want).max() / np.abs(want).max()
                print(f"[weighted k1] {name} {flavour}/{key}: max err / max |want| = {err:.2e}")
                np.testing.assert_allclose(out[key], want, rtol=RTOL, atol=ATOL * np.abs(want).max(), err_msg=f"{name} {flavour} {key}")
                assert np.abs(out[key][:, cols] - plain[:, cols]).max() > NOT_IGNORED      # the weights are not ignored
        if "rows" in out and "tiled" in out:
            assert np.array_equal(out["rows"], out["tiled"])
        if "aux" in out:
            R = out["aux"][:, :9].reshape(B, 3, 3)
            np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), (B, 3, 3)), atol=5e-6)
            np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=5e-6)
            # the centroid rows hold the WEIGHTED centroid
            what = layer.align_w.double().cpu().numpy()
            c = (what[None, :, None] * traj[:, align].astype(np.float64)).mean(1)
            np.testing.assert_allclose(out["aux"][:, 9:12], c, rtol=0, atol=2e-6 * np.abs(traj).max())
        if "slots" in out:
            assert np.array_equal(out["slots"], traj[:, layer.slot_atom.cpu().numpy()].reshape(B, -1))
    # equal weights reproduce the unweighted layer's features (another summation: not bitwise)
    flavour = flavours[-1] if flavours == ("rows",) else "both"
    key = "rows"
    same = weighted_layer(n, align, ref, feats, np.full(len(align), 0.7), dev)
    uni = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    got_same = _run(same, same.pp_desc(), x, B, flavour, dev)[key]
    got_uni = _run(uni, uni.pp_desc(), x, B, flavour, dev)[key]
    np.testing.assert_allclose(got_same, got_uni, rtol=RTOL, atol=ATOL * np.abs(got_uni).max())
    np.testing.assert_allclose(got_uni, plain, rtol=RTOL, atol=ATOL * np.abs(plain).max())


def test_route_at_the_config5_shape_names_slice_with_weights_and_pipe_without(dev):
    """5000 atoms, the benchmark's feature list, 100 000 frames of tiled features: the uniform layer takes the pipelined kernel,
    the weighted one the slice kernel (NI = 3) - no launch, host arithmetic."""
    import bench
    from colvarsfinder import _hip, pp
    n, B = 5000, 100000
    _, _, ref = frames(n, 1, seed=5)
    feats = bench.c5_features(n)
    lib = _hip.lib()
    uni = pp.AlignFeatureLayer(n, list(range(n)), ref, feats).to(dev)
    wl = weighted_layer(n, list(range(n)), ref, feats, weights_for(n, n), dev)
    assert lib.cvf_align_feature_route(uni.pp_desc(), B, 1, 0, 0, 0) == _hip.K1_ROUTE_PIPE + 3
    assert lib.cvf_align_feature_route(wl.pp_desc(), B, 1, 0, 0, 0) == _hip.K1_ROUTE_SLICE + 3
    # generator-mode outputs and small batches: the slice kernel either way
    for desc in (uni.pp_desc(), wl.pp_desc()):
        assert lib.cvf_align_feature_route(desc, B, 1, 0, 1, 1) == _hip.K1_ROUTE_SLICE + 3
        assert lib.cvf_align_feature_route(desc, 16000, 1, 0, 0, 0) == _hip.K1_ROUTE_SLICE + 3
    # a weight table that is not 16-byte aligned takes the scalar capture instance
    d = wl.pp_desc()
    d.align_w = wl.align_w.data_ptr() + 4
    d.n_align -= 4
    assert lib.cvf_align_feature_route(d, B, 1, 0, 0, 0) == _hip.K1_ROUTE_CAPTURE
