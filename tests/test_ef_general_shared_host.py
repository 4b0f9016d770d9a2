"""CPU (-m "not gpu"): the host-side answers of the shared-trunk entries of csrc/ef_general.hip (cvf_ef_general_shared_*, DESIGN.md
section 4.12) - which descriptions the predicate takes and what it says of the others, the workspace formula, and the flat
layout RegAutoEncoderTask's inner task uses (core._SharedTrunkFlat)."""
import pytest

from tests import codeobj


@pytest.fixture(scope="module")
def H():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _flat(dims, k, ns, act=1):
    import torch
    from colvarsfinder import core
    L = len(dims) - 1
    return core._SharedTrunkFlat(dims, [act] * (L - 1) + [0], k, ns, torch.device("cpu"))


@pytest.mark.parametrize("dims,k,ns", [([7, 65, 33, 1], 3, 1), ([9, 130, 1], 2, 1), ([5, 5, 70, 6, 1], 8, 2), ([66, 128, 128, 128, 128, 1], 2, 2),
                                       ([30, 4096, 4096, 1], 8, 2), ([30] + [16] * 11 + [1], 2, 11), ([7, 65, 33, 1], 3, 0), ([7, 65, 1], 1, 1)])
def test_layout_and_predicate_agree(H, dims, k, ns):
    fl = _flat(dims, k, ns)
    L = len(dims) - 1
    size = [dims[l + 1] * (dims[l] + 1) for l in range(L)]
    assert fl.n == sum(size[:ns]) + k * sum(size[ns:]) == fl.desc.n_params
    assert H.lib().cvf_ef_general_shared_supported(fl.desc, ns) == 1, H.lib().cvf_last_error()
    # the plain predicate takes the description exactly when nothing is stored once
    assert H.lib().cvf_ef_general_supported(fl.desc) == (1 if ns == 0 or k == 1 else 0)


def test_workspace_formula_and_what_sharing_saves(H):
    """saved = 64 T (sum_l<ns d_l + k (sum_l>=ns d_l + 2 sum_l d_l + 2)) floats over the hidden widths d_l: the trunk's h_l once."""
    lib = H.lib()
    for dims, k, ns in (([66, 128, 128, 128, 128, 1], 2, 2), ([5, 5, 70, 6, 1], 8, 2), ([9, 130, 1], 2, 1)):
        hid, T = dims[1:-1], 313
        want = 64 * T * (sum(hid[:ns]) + k * (sum(hid[ns:]) + 2 * sum(hid) + 2))
        assert lib.cvf_ef_general_shared_saved_floats(_flat(dims, k, ns).desc, T, ns) == want
        copies = _flat(dims, k, 0)
        assert lib.cvf_ef_general_shared_saved_floats(copies.desc, T, 0) == lib.cvf_ef_general_saved_floats(copies.desc, T, 0) \
            == want + 64 * T * (k - 1) * sum(hid[:ns])
        assert lib.cvf_ef_general_shared_slab_rows(copies.desc, T, 0) == lib.cvf_ef_general_slab_rows(copies.desc, T)
    big = _flat([66, 4096, 4096, 1], 8, 2)
    assert lib.cvf_ef_general_shared_slab_rows(big.desc, 313, 2) == (128 << 20) // (4 * big.n) >= 1


@pytest.mark.parametrize("edit,ns,why", [
    (lambda d: setattr(d, "n_params", d.n_params + 1), 1, "flat buffer holds"),
    (lambda d: d.w_off[1].__setitem__(0, d.w_off[1][0] + 1), 1, "offsets differ"),
    (lambda d: d.b_off[2].__setitem__(0, 3), 1, "offsets differ"),
    (lambda d: d.w_off[2].__setitem__(1, d.w_off[1][1]), 1, "overlap"),
    (lambda d: d.b_off[0].__setitem__(2, d.n_params - 1 + 1), 1, "outside the flat buffer"),
    (lambda d: None, -1, "n_shared"), (lambda d: None, 3, "n_shared"),
    (lambda d: None, 2, "offsets differ"),                        # laid out for one shared layer, asked for two
    (lambda d: d.dims.__setitem__(2, 4097), 1, "4096 units"),
    (lambda d: setattr(d, "n_nets", 9), 1, "nets"),
    (lambda d: d.act.__setitem__(2, 1), 1, "activation after the output"),
])
def test_refusals_say_why(H, edit, ns, why):
    d = _flat([7, 65, 33, 1], 3, 1).desc
    edit(d)
    lib = H.lib()
    assert lib.cvf_ef_general_shared_supported(d, ns) == 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()
    assert lib.cvf_ef_general_shared_saved_floats(d, 4, ns) == 0 and lib.cvf_ef_general_shared_slab_rows(d, 4, ns) == 0


def test_entries_refuse_before_any_launch(H):
    """No GPU here: a refused call must return its negative code without touching the device (NULL buffers are never read)."""
    lib = H.lib()
    fl = _flat([7, 65, 33, 1], 3, 1)
    cfg = H.EFCfg()
    cfg.k, cfg.lag_idx = 3, 2
    assert lib.cvf_ef_general_shared_backward(cfg, fl.desc, 1, None, 70, None, None, None, None, None, None, None, None, None) < 0
    assert "transfer-mode" in lib.cvf_last_error().decode()
    assert lib.cvf_ef_general_shared_fwd(fl.desc, 1, None, None, 2, None, None, None, None) < 0
    assert "transfer-mode" in lib.cvf_last_error().decode()
    assert lib.cvf_ef_general_shared_fwd(fl.desc, 3, None, None, 2, None, None, None, None) < 0
    assert "n_shared" in lib.cvf_last_error().decode()


def test_public_eigenfunction_task_signature_keeps_the_option_private():
    import inspect
    import __graft_entry__  # noqa: F401
    from colvarsfinder import core
    ef = list(inspect.signature(core.EigenFunctionTask.__init__).parameters)
    assert ef[-2:] == ["general_nets", "_shared_trunk"]
    reg = inspect.signature(core.RegAutoEncoderTask.__init__).parameters
    assert list(reg)[-1] == "general_nets" and reg["general_nets"].default is False
