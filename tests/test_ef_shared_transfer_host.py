"""CPU (-m "not gpu"): colvarsfinder.nn.SharedEigenFunctions - the model's contract - and the host-side answers of the transfer-mode
shared-trunk entries of csrc/ef_general.hip (cvf_ef_general_shared_transfer_*): the flat layout the model
gives, the workspace formula, every refusal with NULL buffers, the symbols, and the separation of the GPU cases' eigenvalues."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import codeobj
from tests import ef_shared_transfer_cases as S

NEW = ["cvf_ef_general_shared_transfer_supported", "cvf_ef_general_shared_transfer_saved_floats",
       "cvf_ef_general_shared_transfer_slab_rows", "cvf_ef_general_shared_transfer_fwd", "cvf_ef_general_shared_transfer_backward"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _model(trunk, head, k, act=None, dtype=torch.float32):
    from colvarsfinder import nn
    torch.manual_seed(3)
    return nn.SharedEigenFunctions(trunk, head, k, *([] if act is None else [act])).to(dtype)


SHAPES = [([7, 65], [65, 33, 1], 3), ([9, 130], [130, 1], 2), ([7, 65, 33], [33, 1], 3), ([5, 5, 70], [70, 6, 1], 8), ([4, 6], [6, 1], 1)]


@pytest.mark.parametrize("trunk,head,k", SHAPES)
def test_model_contract(H, trunk, head, k):
    from colvarsfinder import nn
    m = _model(trunk, head, k)
    assert isinstance(m, nn.EigenFunctions) and len(m.eigen_funcs) == k and m.n_shared == len(trunk) - 1
    size = lambda d: sum(b * (a + 1) for a, b in zip(d[:-1], d[1:]))   # noqa: E731
    params = list(m.parameters())
    assert len(params) == 2 * (len(trunk) - 1) + 2 * k * (len(head) - 1)          # every trunk tensor once
    assert sum(p.numel() for p in params) == size(trunk) + k * size(head)
    for l in range(m.n_shared):
        assert all(m.eigen_funcs[i][2 * l] is m.eigen_funcs[0][2 * l] for i in range(k))
    # get_params_of_cv: the trunk's and head i's parameters, by name and identity
    L = len(trunk) + len(head) - 2
    for i in range(k):
        got = m.get_params_of_cv(i)
        assert [n for n, _ in got] == [f"{l + 1}.{n}" for l in range(L) for n in ("weight", "bias")]
        lins = [mod for mod in m.eigen_funcs[i] if isinstance(mod, torch.nn.Linear)]
        assert all(p is q for (_, p), q in zip(got, [t for lin in lins for t in (lin.weight, lin.bias)]))
        if i > 0:
            mine, first = [p for _, p in got], [p for _, p in m.get_params_of_cv(0)]
            assert all(a is b for a, b in zip(mine[:2 * m.n_shared], first)) and not any(a is b for a, b in zip(mine[2 * m.n_shared:], first[2 * m.n_shared:]))
    # state_dict round trip into a differently initialised model
    torch.manual_seed(99)
    m2 = nn.SharedEigenFunctions(trunk, head, k)
    assert any(not torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    m2.load_state_dict(m.state_dict())
    assert list(m.state_dict()) == list(m2.state_dict()) and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    # a deep copy keeps the sharing, and shares nothing with the original
    c = copy.deepcopy(m)
    assert len(list(c.parameters())) == len(params) and not any(a is b for a, b in zip(c.parameters(), params))
    assert all(c.eigen_funcs[i][0] is c.eigen_funcs[0][0] for i in range(k))
    with torch.no_grad():
        c.eigen_funcs[0][0].weight.add_(1.0)
    assert torch.equal(c.eigen_funcs[k - 1][0].weight, c.eigen_funcs[0][0].weight) and not torch.equal(c.eigen_funcs[0][0].weight, m.eigen_funcs[0][0].weight)


def test_constructor_asserts():
    import __graft_entry__  # noqa: F401
    from colvarsfinder import nn
    for trunk, head in (([7, 5], [5, 2]), ([7, 5], [4, 1]), ([7], [7, 1]), ([7, 5], [5])):
        with pytest.raises(AssertionError):
            nn.SharedEigenFunctions(trunk, head, 2)


@pytest.mark.parametrize("trunk,head,k", SHAPES[:4])
def test_forward_equals_eigenfunctions_on_copies_of_the_trunk(H, trunk, head, k):
    """fp64, exact: an EigenFunctions of the full chain loaded with the shared model's state_dict (the trunk copied k times)."""
    from colvarsfinder import nn
    m = _model(trunk, head, k, dtype=torch.float64)
    plain = nn.EigenFunctions(trunk + head[1:], k).double()
    plain.load_state_dict(m.state_dict())
    assert len(list(plain.parameters())) > len(list(m.parameters())) or k == 1
    x = torch.randn(37, trunk[0], dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    y = m(x)
    assert y.shape == (37, k) and torch.equal(y, plain(x))


@pytest.mark.parametrize("trunk,head,k", SHAPES)
def test_flat_layout_is_the_shared_description(H, trunk, head, k):
    """mlp_layout of the model = core._SharedTrunkFlat's description (the trunk once, then head by head), which both predicates take."""
    from colvarsfinder import core
    m = _model(trunk, head, k)
    before = [p.detach().clone() for p in m.parameters()]
    fl = core._FlatParams(m, torch.device("cpu"))
    dims, ns = trunk + head[1:], len(trunk) - 1
    want = core._SharedTrunkFlat(dims, [1] * (len(dims) - 2) + [0], k, ns, torch.device("cpu"))
    assert fl.n == want.n == fl.desc.n_params and fl.packed is None
    assert [fl.desc.dims[i] for i in range(len(dims))] == dims and [fl.desc.act[i] for i in range(len(dims) - 1)] == [1] * (len(dims) - 2) + [0]
    for i in range(k):
        for l in range(len(dims) - 1):
            assert (fl.desc.w_off[i][l], fl.desc.b_off[i][l]) == (want.desc.w_off[i][l], want.desc.b_off[i][l]), (i, l)
    lib = H.lib()
    assert lib.cvf_ef_general_shared_supported(fl.desc, ns) == 1, lib.cvf_last_error()
    assert lib.cvf_ef_general_shared_transfer_supported(fl.desc, ns) == 1, lib.cvf_last_error()
    # the module aliases the buffer: same values, and a write to theta shows in the module
    assert torch.equal(fl.theta, torch.cat([p.reshape(-1) for p in before]))
    fl.theta.add_(1.0)
    assert all(torch.equal(p, b + 1.0) for p, b in zip(m.parameters(), before))
    assert [id(p) for p, _ in fl.grad_views()] == [id(p) for p in m.parameters()]


def _flat(dims, k, ns, act=1):
    from colvarsfinder import core
    return core._SharedTrunkFlat(dims, [act] * (len(dims) - 2) + [0], k, ns, torch.device("cpu"))


def test_saved_floats_formula_and_what_sharing_saves(H):
    """saved = 64 n_tiles (sum_l<ns d_l + k (sum_l>=ns d_l + 2 max_l d_l + 1)) floats over the hidden widths d_l: the trunk's h_l once."""
    lib = H.lib()
    for dims, k, ns in [(c[1], c[2], c[3]) for c in S.CASES] + [([66, 128, 128, 128, 128, 1], 3, 2)]:
        hid, nt = dims[1:-1], 2 * 313
        want = 64 * nt * (sum(hid[:ns]) + k * (sum(hid[ns:]) + 2 * max(hid) + 1))
        assert lib.cvf_ef_general_shared_transfer_saved_floats(_flat(dims, k, ns).desc, nt, ns) == want
        copies = _flat(dims, k, 0)
        plain = lib.cvf_ef_general_saved_floats(copies.desc, nt, 2)
        assert lib.cvf_ef_general_shared_transfer_saved_floats(copies.desc, nt, 0) == plain == want + 64 * nt * (k - 1) * sum(hid[:ns])
        assert want < plain
        assert lib.cvf_ef_general_shared_transfer_slab_rows(copies.desc, nt, 0) == lib.cvf_ef_general_slab_rows(copies.desc, nt)
        assert lib.cvf_ef_general_shared_transfer_slab_rows(_flat(dims, k, ns).desc, nt, ns) == min(256, nt, (128 << 20) // (4 * _flat(dims, k, ns).n))
    assert lib.cvf_ef_general_shared_transfer_saved_floats(_flat([7, 65, 33, 1], 3, 1).desc, 0, 1) == 0


def test_every_refusal_with_null_buffers_names_its_reason(H):
    """No GPU here: a refused call returns its negative code without touching the device (NULL buffers are never read)."""
    lib = H.lib()
    dims, k, ns = [7, 65, 33, 1], 3, 1
    fl = _flat(dims, k, ns)
    tr, gen = H.EFCfg(), H.EFCfg()
    tr.k, tr.lag_idx, gen.k, gen.lag_idx = k, 2, k, 0
    one = torch.ones(1)   # a non-NULL host address that a refused call must not read either
    p1 = ctypes.c_void_p(one.data_ptr())

    def bwd(cfg, d, n, w_lag=None):
        return lib.cvf_ef_general_shared_transfer_backward(cfg, d, n, None, 70, None, w_lag, None, None, None, None, None, None, None)

    def fwd(d, n):
        return lib.cvf_ef_general_shared_transfer_fwd(d, n, None, None, 4, None, None, None)

    def says(why):
        assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()

    assert bwd(gen, fl.desc, ns, p1) < 0
    says("generator-mode cfg")
    assert bwd(tr, fl.desc, ns, None) < 0
    says("needs w_lag")
    for n in (-1, 3):
        assert lib.cvf_ef_general_shared_transfer_supported(fl.desc, n) == 0
        says("n_shared")
        assert lib.cvf_ef_general_shared_transfer_saved_floats(fl.desc, 4, n) == 0 and lib.cvf_ef_general_shared_transfer_slab_rows(fl.desc, 4, n) == 0
        assert fwd(fl.desc, n) < 0
        says("n_shared")
        assert bwd(tr, fl.desc, n, p1) < 0
        says("n_shared")
    d = _flat(dims, k, ns).desc
    d.w_off[1][0] += 1
    assert lib.cvf_ef_general_shared_transfer_supported(d, ns) == 0
    says("offsets differ")
    assert fwd(d, ns) < 0
    says("offsets differ")
    assert bwd(tr, d, ns, p1) < 0
    says("offsets differ")
    assert lib.cvf_ef_general_shared_transfer_saved_floats(d, 4, ns) == 0
    assert fwd(fl.desc, ns) < 0      # a good description, NULL buffers
    says("bad argument")
    assert bwd(tr, fl.desc, ns, p1) < 0
    says("bad argument")
    assert lib.cvf_ef_general_shared_transfer_supported(fl.desc, ns) == 1
    # the generator-mode shared entries keep refusing transfer mode by name
    assert lib.cvf_ef_general_shared_backward(tr, fl.desc, ns, None, 70, None, None, None, None, None, None, None, None, None) < 0
    says("transfer-mode")
    assert lib.cvf_ef_general_shared_fwd(fl.desc, ns, None, None, 2, None, None, None, None) < 0
    says("transfer-mode")


def test_new_symbols_are_declared_bound_and_exported(H):
    header = open(os.path.join(ROOT, "include", "cvf.h")).read()
    handle = H.lib()
    for name in NEW:
        assert re.search(r"^(int|int64_t) " + name + r"\(", header, re.M), name
        assert name in H._SIGNATURES and name in H.EXPORTED_SYMBOLS and hasattr(handle, name), name


def test_kernels_of_the_transfer_step_fit_the_budget(H, tmp_path):
    """The two summing kernels: no scratch, no spills, at most 96 VGPRs; the four efg_ kernels keep their
    code object to themselves and eftr_top_sum_kernel."""
    objs = codeobj.built_objects()
    found = {}
    for obj in ("ef_general.o", "ef_general_sum.o"):
        for n, v in codeobj.kernels_of(os.path.join(objs, obj), tmp_path).items():
            if "eftr_" in n:
                found[n] = v
    assert len(found) == 2 and any("eftr_trunk_sum_kernel" in n for n in found) and any("eftr_top_sum_kernel" in n for n in found), list(found)
    for n, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v["vgpr_count"] <= 96, (n, v)


def test_eigenvalues_are_separated():
    """Every GPU case's fp64 eigenvalues differ pairwise by more than 20 x the eigenvalue bar (relative; the bar is 8 x the fp32
    oracle's own error, so 160 x that error): cvec is decided."""
    ref, bars = S.reference()
    assert all(0 < b < 1e-2 for b in bars.values()), bars
    for (cid, B), (lv, eig, cvec, grad) in ref.items():
        gaps = np.diff(np.sort(eig)) / np.abs(eig).max()
        print(f"[shared-tr] {cid} B={B}: smallest eigenvalue gap {gaps.min():.2e} (eig bar {bars['eig']:.2e})")
        assert gaps.min() > 20 * bars["eig"], (cid, B, eig)
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0
