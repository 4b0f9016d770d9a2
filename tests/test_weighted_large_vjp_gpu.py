"""GPU (-m gpu): the vector-Jacobian product of a WEIGHTED alignment on frames of more than 64 atoms
(``vjp_weighted_large_kernel`` / ``vjp_rows_weighted_large_kernel``, csrc/k1_vjp_large.hpp: d_b = Z ref_b - w_b shift) against autograd through the fp64 oracle, at
``LARGE_TOL`` of tests/test_align_vjp_gpu.py; ``gx`` starts as NaN and must come back fully written; row i of the k-row call is
bit for bit the single call on ``g[:, i]``; and the layer as an autograd node on a CPU fp64 input."""
import numpy as np
import pytest
import torch

from tests.test_align_vjp_gpu import LARGE_TOL, abi, case, rel_err
from tests.test_cv_jacobian_gpu import abi_rows
from tests.weighted_large_cases import frames, oracle_layer, weighted_layer, weights_for

pytestmark = pytest.mark.gpu

CASES = [("mixed65", 64), ("mixed1000", 130)]   # 65 atoms / 32 align atoms; 1000 atoms / 600 align atoms (partial, non-contiguous sets)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _build(name, B, dev):
    n, align, feats, _ = case(name)
    traj, _, ref = frames(n, B, seed=700 + n)
    w = weights_for(n, len(align))
    return n, align, feats, w, traj, ref, weighted_layer(n, align, ref, feats, w, dev)


def _oracle_vjp(align, ref, feats, w, traj, g):
    """gx [B, k, 3N] of the cotangents g [B, k, d_r] through the fp64 oracle."""
    torch.set_default_dtype(torch.float64)
    try:
        x = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        y = oracle_layer(align, ref, feats, w)(x)
        rows = [torch.autograd.grad(y, x, g[:, i].double(), retain_graph=True)[0] for i in range(g.shape[1])]
    finally:
        torch.set_default_dtype(torch.float32)
    return torch.stack(rows, 1).reshape(len(traj), g.shape[1], -1).numpy()


@pytest.fixture(scope="module")
def reference():
    """Oracle results per case, computed once."""
    out = {}
    for name, B in CASES:
        n, align, feats, _ = case(name)
        traj, _, ref = frames(n, B, seed=700 + n)
        w = weights_for(n, len(align))
        G = torch.randn(B, 3, sum(3 * len(a) if t == "position" else 2 if t == "dihedral" else 1 for t, a in feats),
                        generator=torch.Generator().manual_seed(B + n), dtype=torch.float64)
        out[name] = dict(G=G, want=_oracle_vjp(align, ref, feats, w, traj, G), plain=_oracle_vjp(align, ref, feats, None, traj, G[:, :1]))
    return out


@pytest.mark.parametrize("name,B", CASES)
def test_weighted_vjp_and_rows_vs_oracle(dev, reference, name, B):
    n, align, feats, w, traj, ref, layer = _build(name, B, dev)
    G, want = reference[name]["G"], reference[name]["want"]
    assert G.shape[2] == layer.d_r
    _, gx = abi(layer, traj, G[:, 0])
    got = gx.cpu().numpy()
    assert np.isfinite(got).all(), "gx not fully written"
    err = rel_err(got, want[:, 0])
    print(f"[weighted vjp] {name} B={B}: max err / max |g_ref| = {err:.2e}")
    assert err <= LARGE_TOL, err
    # a kernel that ignored the weights could not pass: the UNWEIGHTED oracle's gradient (a property of the inputs, not of the code
    # under test) lies a hundred bars away from the weighted one
    assert rel_err(reference[name]["plain"][:, 0], want[:, 0]) > 100 * LARGE_TOL
    rows, single = abi_rows(layer, traj, G)
    assert not torch.isnan(rows).any(), "rows not fully written"
    assert torch.equal(rows, single)                       # row i == the single call on g[:, i], bit for bit
    assert torch.equal(single[:, 0], gx)
    err_rows = rel_err(rows.cpu().numpy(), want)
    print(f"[weighted vjp] {name} B={B} k=3 rows: {err_rows:.2e}")
    assert err_rows <= LARGE_TOL, err_rows


def test_weighted_large_layer_backward_on_a_cpu_fp64_input(dev, reference):
    name, B = CASES[0]
    n, align, feats, w, traj, ref, layer = _build(name, B, dev)
    G, want = reference[name]["G"], reference[name]["want"]
    x = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    y = layer(x)
    assert y.dtype == torch.float64 and y.device.type == "cpu"
    y.backward(G[:, 1])
    assert x.grad.dtype == torch.float64 and x.grad.device.type == "cpu" and x.grad.shape == x.shape
    err = rel_err(x.grad.reshape(B, -1).numpy(), want[:, 1])
    print(f"[weighted vjp] layer(x).backward(): {err:.2e}")
    assert err <= LARGE_TOL, err
