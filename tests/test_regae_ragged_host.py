"""CPU (-m "not gpu"): RegAutoEncoderTask with decoder and regulariser nets of different depths - the flat layout
core._RegRaggedFlatParams builds (the dense chain it describes reproduces forward_ae | forward_reg; mask, aliasing, frozen
encoder), the C entries cvf_regae_ragged_* in the header, the binding and the library, cvf_regae_ragged_supported and the
workspace against the Python mirrors of tests/regae_ragged_cases.py, the reasons the refusals give, and the case table of the GPU
module: what it reaches and where its bars come from."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import ae_cases as A
from tests import codeobj
from tests import regae_general_cases as G
from tests import regae_ragged_cases as R

NEW = ("cvf_regae_ragged_supported", "cvf_regae_ragged_scratch_floats", "cvf_regae_ragged_forward", "cvf_regae_ragged_backward",
       "cvf_regae_ragged_backward_reuse")
ACT_FN = {0: lambda x: x, 1: torch.tanh, 2: torch.sigmoid}


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _eval_chain(flat, x, n_enc, n_dec, n_reg, K):
    """The dense chain the layout describes, as the kernels walk it: (reconstruction, heads)."""
    d, L = flat.desc, flat.desc.n_layers
    ls = n_enc + min(n_dec, n_reg)
    fin = K if n_dec > n_reg else d.dims[0]
    h, done = x, None
    for l in range(L):
        fo, fi = d.dims[l + 1], d.dims[l] - (fin if l == ls else 0)
        W = flat.theta[d.w_off[0][l]:d.w_off[0][l] + fo * fi].view(fo, fi)
        b = flat.theta[d.b_off[0][l]:d.b_off[0][l] + fo]
        z = h[:, :fi] @ W.T + b
        h = ACT_FN[d.act[l]](z)
        if l + 1 == ls:                                        # the shallower group ends: its rows take no activation
            done = z[:, fo - fin:]
            h = torch.cat([h[:, :fo - fin], done], dim=1)
    return (h, done) if n_dec > n_reg else (done, h)


@pytest.mark.parametrize("e,dd,r,K,act", [
    ([7, 5, 3], [3, 4, 6, 7], [3, 2, 1], 2, torch.nn.Tanh),             # decoder one deeper
    ([7, 5, 3], [3, 4, 6, 5, 7], [3, 2, 1], 3, torch.nn.Sigmoid),       # two deeper; act(0) != 0
    ([7, 5, 3], [3, 4, 7], [3, 2, 5, 1], 2, torch.nn.Tanh),             # regularisers one deeper
    ([7, 3], [3, 4, 7], [3, 2, 5, 4, 1], 1, torch.nn.Sigmoid),          # two deeper, one net, encoder without hidden layer
    ([7, 5, 3], [3, 4, 6, 7], [3, 1], 2, torch.nn.Tanh),                # Lr = 1
    ([7, 5, 3], [3, 7], [3, 2, 5, 1], 2, torch.nn.Tanh),                # Ld = 1
])
def test_ragged_chain_layout(e, dd, r, K, act):
    """The pattern of test_host_logic.py::test_regautoencoder_side_by_side_chain_layout."""
    from colvarsfinder import core, nn
    torch.manual_seed(4)
    model = nn.RegAutoEncoder(e, dd, r, K, activation=act())
    x = torch.randn(9, e[0])
    want_ae, want_reg = model.forward_ae(x).detach(), model.forward_reg(x).detach()
    n_real = sum(p.numel() for p in model.parameters())
    flat = core._RegRaggedFlatParams(model, torch.device("cpu"))
    d, n_enc, n_dec, n_reg = flat.desc, len(e) - 1, len(dd) - 1, len(r) - 1
    assert (flat.n_dec, flat.n_reg, flat.K, flat.dec_deep) == (n_dec, n_reg, K, n_dec > n_reg)
    assert (d.n_nets, d.n_layers) == (1, n_enc + max(n_dec, n_reg))
    c = R._case("layout", e[0], e[1:-1], e[-1], dd[1:-1], r[1:-1], K, 9, 0, 1)
    dims, cols, ls, fin, dec_deep = R.shape(c)
    assert [d.dims[i] for i in range(d.n_layers + 1)] == dims and d.n_params == flat.n == R.n_params(c)
    assert d.dims[d.n_layers] == (e[0] if dec_deep else K) and max(cols) <= max(dims)      # no column for a finished row
    code = 1 if act is torch.nn.Tanh else 2
    assert [d.act[i] for i in range(d.n_layers)] == [0 if l in (n_enc - 1, d.n_layers - 1) else code for l in range(d.n_layers)]
    rec, heads = _eval_chain(flat, x, n_enc, n_dec, n_reg, K)
    torch.testing.assert_close(rec, want_ae, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(heads, want_reg, rtol=1e-6, atol=1e-6)
    assert int(flat.mask.sum()) == n_real and set(flat.mask.unique().tolist()) <= {0.0, 1.0}
    dead = flat.mask == 0
    assert not bool(dead.any()) or float(flat.theta[dead].abs().max()) == 0.0
    assert flat.n >= n_real and (flat.n > n_real) == bool(dead.any())
    assert len(flat.grad_views()) == len(list(model.parameters()))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == \
           {k: tuple(v.shape) for k, v in nn.RegAutoEncoder(e, dd, r, K).state_dict().items()}
    # aliasing, both ways: through the module into the flat buffer, through the flat buffer into the module
    for p, tv, gv in flat.views:
        assert p.data_ptr() == tv.data_ptr() and tv.shape == p.shape == gv.shape
    before = flat.theta.clone()
    with torch.no_grad():
        model.reg[K - 1]._modules[str(len(r) - 1)].weight.add_(1.0)
        model.decoder._modules[str(len(dd) - 1)].bias.add_(2.0)
    changed = (flat.theta != before)
    assert int(changed.sum()) == r[-2] + dd[-1] and bool((flat.mask[changed] == 1).all())
    rec2, heads2 = _eval_chain(flat, x, n_enc, n_dec, n_reg, K)
    torch.testing.assert_close(rec2, model.forward_ae(x).detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(heads2, model.forward_reg(x).detach(), rtol=1e-6, atol=1e-6)
    with torch.no_grad():
        flat.theta.mul_(flat.mask * 0.5)
    torch.testing.assert_close(_eval_chain(flat, x, n_enc, n_dec, n_reg, K)[0], model.forward_ae(x).detach(), rtol=1e-6, atol=1e-6)
    # frozen encoder: its entries leave the mask
    model2 = nn.RegAutoEncoder(e, dd, r, K, activation=act())
    flat2 = core._RegRaggedFlatParams(model2, torch.device("cpu"), freeze_encoder=True)
    n_encp = sum(p.numel() for p in model2.encoder.parameters())
    assert int(flat2.mask.sum()) == n_real - n_encp and float(flat2.mask[:n_encp].sum()) == 0.0


def test_layout_refusals_name_their_reason():
    from colvarsfinder import core, nn
    cpu = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="same number of layers"):      # the side-by-side layout keeps refusing
        core._RegFlatParams(nn.RegAutoEncoder([7, 5, 3], [3, 4, 7], [3, 4, 4, 1], 1), cpu)
    with pytest.raises(AssertionError, match="equal depths"):
        core._RegRaggedFlatParams(nn.RegAutoEncoder([7, 5, 3], [3, 4, 7], [3, 4, 1], 1), cpu)
    model = nn.RegAutoEncoder([7, 5, 3], [3, 4, 7], [3, 4, 4, 1], 2)
    model.reg[1] = nn.create_sequential_nn([3, 5, 4, 1])
    with pytest.raises(NotImplementedError, match="share one reg_layer_dims"):
        core._RegRaggedFlatParams(model, cpu)
    model = nn.RegAutoEncoder([7, 5, 3], [3, 4, 7], [3, 4, 4, 1], 1)
    model.decoder = nn.create_sequential_nn([3, 4, 7], torch.nn.ReLU())
    with pytest.raises(NotImplementedError, match="share the activation"):
        core._RegRaggedFlatParams(model, cpu)
    with pytest.raises(AssertionError, match="at most 12 layers"):
        core._RegRaggedFlatParams(nn.RegAutoEncoder([7, 5, 3], [3] + [4] * 10 + [7], [3, 4, 1], 1), cpu)


def test_header_binding_and_exports_agree(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and hasattr(handle, name) and hasattr(hip.lib(), name), name
    assert set(hip._SIGNATURES) == declared
    # the calls take the argument lists of their equal-depth twins with the two depths behind n_enc_layers
    arglist = lambda name: re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)).strip()
    for tail in ("supported", "forward", "backward", "backward_reuse"):
        new, old = arglist("cvf_regae_ragged_" + tail), arglist("cvf_regae_general_" + tail)
        assert new == old.replace("int n_enc_layers", "int n_enc_layers, int n_dec_layers, int n_reg_layers"), tail
        a, b = hip._SIGNATURES["cvf_regae_ragged_" + tail], hip._SIGNATURES["cvf_regae_general_" + tail]
        at = max(i for i, t in enumerate(b[1]) if t is C.c_int) + 1          # behind n_enc_layers, the last int of these lists
        assert a[0] is b[0] and list(a[1]) == list(b[1][:at]) + [C.c_int, C.c_int] + list(b[1][at:]), tail
    comment = open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read()
    assert "core.py:884-897, 975-1034, 1066-1128" in comment[comment.index("DIFFERENT depths"):comment.index("cvf_regae_ragged_supported")]


def test_supported_and_workspace_equal_the_mirrors(hip):
    lib = hip.lib()
    for c in R.CASES:
        m, (ne, nd, nr) = R.mlp_desc(c), R.depths(c)
        assert lib.cvf_regae_ragged_supported(m, c.K, ne, nd, nr) == 1, (c.id, lib.cvf_last_error())
        assert R.supported(R.shape(c)[0], c.K, ne, nd, nr, R.acts(c), R.n_params(c)), c.id
        for B in (1, c.B, 2 * c.B, 20_000):
            assert lib.cvf_regae_ragged_scratch_floats(m, B, c.K, ne, nd, nr) == R.scratch_floats(c, B) > 0, (c.id, B)
        assert lib.cvf_regae_ragged_scratch_floats(m, 0, c.K, ne, nd, nr) == 0
        assert lib.cvf_regae_ragged_scratch_floats(m, c.B, c.K, ne, nr, nd) == 0          # the depths swapped
        # the equal-depth route refuses the same description, and the fused one has no layout for it
        assert lib.cvf_regae_general_supported(m, c.K, ne) == 0, c.id
    dip = next(c for c in R.CASES if c.id == "dipeptide-small-regularisers")
    assert R.shape(dip)[:4] == ([66, 128, 128, 2, 168, 130, 66], [66, 128, 128, 2, 168, 128], 5, 2)
    assert 4 * R.scratch_floats(dip, 20_000) < 1 << 30


def _good():
    return next(c for c in R.CASES if c.id == "decoder-one-deeper"), next(c for c in R.CASES if c.id == "regularisers-one-deeper")


@pytest.mark.parametrize("which,edit,why", [
    (0, dict(K=9), "K = 9"),
    (0, dict(K=0), "K = 0"),
    (0, dict(nd=2), "two different depths"),
    (0, dict(nr=0), "two different depths"),
    (0, dict(ne=1), "is not the chain's 5 layers"),
    (0, dict(act_enc=1), "the encoder's last layer must have no activation"),
    (0, dict(latent=9), "latent width 9 > 8"),
    (0, dict(last=7), "must end in the deeper group's 6 outputs (it has 7)"),
    (1, dict(last=3), "must end in the deeper group's 2 outputs (it has 3)"),
    (0, dict(ls_width=2), "leave no row for the deeper one"),
    (0, dict(n_params=1), "outside the chain"),
    (1, dict(w_off=10_000), "outside the flat buffer"),
    (1, dict(width=4097), "4096 units"),
    (1, dict(n_nets=2), "2 nets"),
])
def test_refused_chains_say_why(hip, which, edit, why):
    """Every refusal names its reason and launches nothing (no device is touched: this runs without a GPU)."""
    lib, c = hip.lib(), _good()[which]
    m, (ne, nd, nr), K = R.mlp_desc(c), R.depths(c), c.K
    dims, n_par = R.shape(c)[0], R.n_params(c)
    K, ne, nd, nr = edit.get("K", K), edit.get("ne", ne), edit.get("nd", nd), edit.get("nr", nr)
    if "act_enc" in edit:
        m.act[ne - 1] = edit["act_enc"]
    if "latent" in edit:
        m.dims[ne] = dims[ne] = edit["latent"]
    if "last" in edit:
        m.dims[m.n_layers] = dims[-1] = edit["last"]
    if "ls_width" in edit:
        m.dims[ne + min(nd, nr)] = dims[ne + min(nd, nr)] = edit["ls_width"]
    if "width" in edit:
        m.dims[1] = dims[1] = edit["width"]
    if "n_params" in edit:
        m.n_params += edit["n_params"]
        n_par += edit["n_params"]
    if "w_off" in edit:
        m.w_off[0][2] = edit["w_off"]
    if "n_nets" in edit:
        m.n_nets = edit["n_nets"]
    assert lib.cvf_regae_ragged_supported(m, K, ne, nd, nr) == 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error().decode()
    if "w_off" not in edit and "n_nets" not in edit:
        assert not R.supported(dims, K, ne, nd, nr, [m.act[l] for l in range(m.n_layers)], n_par)
    assert lib.cvf_regae_ragged_scratch_floats(m, 70, K, ne, nd, nr) == 0
    assert lib.cvf_regae_ragged_forward(m, None, None, None, 1, 0, 0, K, None, None, None, ne, nd, nr, None, None, None) < 0
    assert why in lib.cvf_last_error().decode()
    for bwd in (lib.cvf_regae_ragged_backward, lib.cvf_regae_ragged_backward_reuse):
        assert bwd(m, None, None, None, 1, 0, 0, K, None, None, 1.0, 1.0, None, None, ne, nd, nr, None, None, None, None, None, None, None) < 0
        assert why in lib.cvf_last_error().decode()


def test_good_chain_with_missing_buffers_or_a_negative_lag_is_refused(hip):
    lib = hip.lib()
    for c in _good():
        m, (ne, nd, nr) = R.mlp_desc(c), R.depths(c)
        assert lib.cvf_regae_ragged_forward(m, None, None, None, 1, 0, 1, c.K, None, None, None, ne, nd, nr, None, None, None) < 0
        assert "bad argument" in lib.cvf_last_error().decode()
        assert lib.cvf_regae_ragged_forward(m, None, None, None, 1, -1, 1, c.K, None, None, None, ne, nd, nr, None, None, None) < 0
        assert "negative lag" in lib.cvf_last_error().decode()
    assert lib.cvf_regae_ragged_supported(None, 1, 1, 1, 2) == 0 and "no chain description" in lib.cvf_last_error().decode()
    for a in range(0, 7):
        m = R.mlp_desc(_good()[0])
        m.act[2] = m.act[3] = a
        assert lib.cvf_regae_ragged_supported(m, 2, 2, 3, 2) == 1
    m.act[2] = 7
    assert lib.cvf_regae_ragged_supported(m, 2, 2, 3, 2) == 0 and "activation" in lib.cvf_last_error().decode()


def test_no_kernel_was_added_for_the_route(hip, tmp_path):
    """The ragged calls launch the kernels of the equal-depth route (regaeg_out_kernel takes the reconstruction and the heads as two
    views): the same six kernels in the code object, each without scratch or spills and within 128 registers."""
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "regae_general.o"), tmp_path)
    assert len(kernels) == 6 and sum("regaeg_out_kernel" in n for n in kernels) == 1, sorted(kernels)
    for n, v in kernels.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)


def test_the_table_reaches_its_edges():
    cases = R.CASES
    ids = {c.id: c for c in cases}
    assert len(ids) == len(cases) <= 16
    with_grad = [c for c in cases if R.grad(c)]
    gap = lambda c: len(c.dec) - len(c.reg)
    assert {gap(c) for c in with_grad} >= {-2, -1, 1, 2}
    assert any(len(c.reg) == 0 and gap(c) > 0 for c in with_grad) and any(len(c.dec) == 0 and gap(c) < 0 for c in with_grad)
    heads_astride = [c for c in with_grad if gap(c) > 0 and R.shape(c)[0][R.shape(c)[2]] - c.K < 64 < R.shape(c)[0][R.shape(c)[2]]]
    assert heads_astride and any((c.lag_ae, c.lag_reg, c.B, c.idx) == (70, 67, 130, True) for c in heads_astride)
    rec_astride = [c for c in with_grad if gap(c) < 0 and c.d > 64 > R.shape(c)[0][R.shape(c)[2]] - c.d]
    assert rec_astride
    assert all(c.B % A.TILE for c in cases) and {G.n_tiles(c.B) for c in with_grad} >= {2, 3}
    for a in ("relu", "sigmoid"):
        assert {gap(c) > 0 for c in with_grad if R.act(c) == a} == {True, False}
    assert R.FROZEN <= set(ids) and R.ADAM <= {c.id for c in with_grad} and set(R.ACT) <= set(ids) and R.LOSS_ONLY <= set(ids)
    dip = ids["dipeptide-small-regularisers"]
    assert R.model_dims(dip) == ([66, 128, 128, 2], [2, 128, 128, 66], [2, 20, 1]) and dip.B == 130 and dip.idx
    assert all(c.K <= 2 for c in cases if abs(gap(c)) == 2 or not c.dec)       # the ill-conditioned directions stay on K <= 2
    assert all(R.act(c) == "tanh" for c in cases if not c.dec or gap(c) == -2)


def test_bars_are_tied_to_the_fp32_oracle():
    """Every bar is 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over the table's cases, per term, recomputed
    here from the table's own inputs: between 4 x and 16 x; and none exceeds the largest bar of the equal-depth routes."""
    worst, where = R.group_e32()
    print({t: (f"{worst[t]:.2e}", where.get(t)) for t in worst})
    assert set(worst) == set(R.BARS) == set(R.TERMS)
    assert R.BAR_CAP == dict(loss=2.0e-5, ae=4.1e-7, npl=1.2e-4, pen=4.5e-8, eig=1.7e-4, norm=1.5e-7, orth=4.0e-5, grad=2.8e-4)
    for term, bar in R.BARS.items():
        assert 4 * worst[term] <= bar <= 16 * worst[term], f"{term}: bar {bar:.2e}, worst e32 {worst[term]:.2e}"
        assert bar <= R.BAR_CAP[term], f"{term}: bar {bar:.2e} above {R.BAR_CAP[term]:.2e}"


def test_adam_cases_are_ones_the_fp32_oracle_itself_meets():
    import numpy as np
    from tests.test_ae_sweep_gpu import ADAM_LR, ADAM_STEPS, ADAM_TOL
    assert R.ADAM_SOURCE_MAX == ADAM_TOL / 8 and {len(c.dec) > len(c.reg) for c in R.CASES if c.id in R.ADAM} == {True, False}
    for c in R.CASES:
        if c.id in R.ADAM:
            inp, ref = R.reference(c, ADAM_STEPS, ADAM_LR)
            with G._fixed_order_fp32():
                p32 = R.oracle(c, inp, torch.float32, ADAM_STEPS, ADAM_LR)[3]
            keep = R.adam_compared(c, inp[4])
            assert int((~keep).sum()) == c.K and float(np.abs(p32 - ref[3])[keep].max()) <= R.ADAM_SOURCE_MAX, c.id
