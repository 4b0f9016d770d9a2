"""CPU (-m "not gpu"): the general eigenfunction route's host-side answers (csrc/ef_general.hip) - which shapes it takes, the
size of its workspace against the bound DESIGN.md section 4.8 states, and the register / scratch budget of its kernels read
from the built code object."""
import ctypes

import pytest

from tests import codeobj

GIB = 1 << 30


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _desc(_hip, dims, k, act=1):
    d = _hip.MLPDesc()
    L = len(dims) - 1
    d.n_nets, d.n_layers = k, L
    pos = 0
    for l in range(L):
        d.dims[l], d.dims[l + 1], d.act[l] = dims[l], dims[l + 1], (act if l < L - 1 else 0)
    for i in range(k):
        for l in range(L):
            d.w_off[i][l], d.b_off[i][l] = pos, pos + dims[l + 1] * dims[l]
            pos += dims[l + 1] * (dims[l] + 1)
    d.n_params = pos
    return d


@pytest.mark.parametrize("dims,k,act", [([30, 128, 128, 1], 2, 1), ([30, 24, 1], 1, 1), ([30] + [20] * 6 + [1], 2, 1),
                                        ([30] + [16] * 11 + [1], 1, 1), ([30, 100, 40, 1], 2, 2), ([30, 72, 33, 17, 1], 2, 6),
                                        ([384, 256, 256, 256, 1], 8, 1), ([30, 1, 1], 1, 3), ([30, 4096, 1], 1, 5)])
def test_supported_shapes(lib, dims, k, act):
    assert lib.lib().cvf_ef_general_supported(_desc(lib, dims, k, act)) == 1


@pytest.mark.parametrize("dims,k,act,why", [([30] + [16] * 12 + [1], 1, 1, "hidden layers"), ([30, 4097, 1], 1, 1, "4096 units"),
                                            ([30, 20, 2], 1, 1, "scalar"), ([30, 20, 1], 9, 1, "nets"), ([30, 20, 1], 1, 7, "activation"),
                                            ([70000, 20, 1], 1, 1, "input features")])
def test_unsupported_shapes_say_why(lib, dims, k, act, why):
    d = _desc(lib, dims if len(dims) <= 13 else dims[:12] + [1], min(k, 8), act)
    d.n_layers = len(dims) - 1   # (13 layers: past what the descriptor can describe)
    if k > 8:
        d.n_nets = k
    assert lib.lib().cvf_ef_general_supported(d) == 0
    assert why in lib.lib().cvf_last_error().decode()


def test_parameters_outside_the_nets_are_refused(lib):
    d = _desc(lib, [30, 40, 1], 2)
    d.n_params += 1
    assert lib.lib().cvf_ef_general_supported(d) == 0
    assert lib.lib().cvf_ef_general_slab_rows(d, 10) == 0 and lib.lib().cvf_ef_general_saved_floats(d, 10, 0) == 0


def test_workspace_bound_at_the_large_shape(lib):
    """[384,256,256,256,1] x 8 nets, B = 20 000: slab + saved activations, sweep of g, tangents and adjoints < 2 GiB in both
    modes."""
    d = _desc(lib, [384, 256, 256, 256, 1], 8)
    T = (20000 + 63) // 64
    for lag, nt in ((0, T), (2, 2 * T)):
        rows = lib.lib().cvf_ef_general_slab_rows(d, nt)
        saved = lib.lib().cvf_ef_general_saved_floats(d, nt, lag)
        assert 1 <= rows <= 256
        assert 4 * (rows * d.n_params + saved) < 2 * GIB, (lag, rows, saved)
    # the slab stays within its 128 MiB budget, and never has more rows than tiles
    assert 4 * lib.lib().cvf_ef_general_slab_rows(d, T) * d.n_params <= 128 << 20
    assert lib.lib().cvf_ef_general_slab_rows(_desc(lib, [30, 40, 1], 1), 3) == 3


def test_kernels_have_no_scratch_and_fit_the_register_budget(lib, tmp_path):
    import os
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "ef_general.o"), tmp_path)
    names = [n for n in kernels if "efg_" in n]
    assert len(names) == 4, names
    for n in names:
        v = kernels[n]
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
        # (256-thread blocks, at most 96 VGPRs - five waves per SIMD)
        assert v["vgpr_count"] <= 96, (n, v)
