"""CPU (-m "not gpu"): the host-side answers of RegAutoEncoderTask's per-layer route (csrc/regae_general.hip) - the route query
cvf_regae_route against ae_cases.mfma_layout, the chains cvf_regae_general_supported takes and the reasons it gives for the
others, its workspace against the Python mirror of tests/regae_general_cases.py, the new C entries in the header, the binding
and the library, the register / scratch budget of its kernels read from the built code object, and the case table of the GPU
module: what it reaches and where its bars come from."""
import ctypes as C
import os
import re

import pytest

from tests import ae_cases as A
from tests import codeobj
from tests import regae_general_cases as G

NEW = ("cvf_regae_route", "cvf_regae_general_supported", "cvf_regae_general_scratch_floats", "cvf_regae_general_forward",
       "cvf_regae_general_backward", "cvf_regae_general_backward_reuse")


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _desc(hip, d, n_enc, act=1):
    """One chain over a flat buffer, W then b per layer; `act` after every layer but the encoder's and the chain's last."""
    m, L, pos = hip.MLPDesc(), len(d) - 1, 0
    m.n_nets, m.n_layers = 1, L
    for l in range(L):
        m.dims[l], m.dims[l + 1], m.act[l] = d[l], d[l + 1], (0 if l in (n_enc - 1, L - 1) else act)
        m.w_off[0][l], pos = pos, pos + d[l] * d[l + 1]
        m.b_off[0][l], pos = pos, pos + d[l + 1]
    m.n_params = pos
    return m


def test_header_binding_and_exports_agree(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and hasattr(handle, name), name
        assert hasattr(hip.lib(), name)
    assert set(hip._SIGNATURES) == declared
    # the calls take the argument lists of the fused ones: _step swaps functions by name
    arglist = lambda name: re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)).strip()
    for new, old in (("cvf_regae_general_forward", "cvf_regae_forward"), ("cvf_regae_general_backward", "cvf_regae_backward"),
                     ("cvf_regae_general_backward_reuse", "cvf_regae_backward_reuse"),
                     ("cvf_regae_general_scratch_floats", "cvf_regae_scratch_floats")):
        assert arglist(new) == arglist(old), new
        assert list(hip._SIGNATURES[new][1]) == list(hip._SIGNATURES[old][1]) and hip._SIGNATURES[new][0] is hip._SIGNATURES[old][0]
    assert os.path.exists(os.path.join(codeobj.CSRC, "regae_general.hip"))


def test_route_query_equals_the_mirror(hip):
    """cvf_regae_route against ae_cases.mfma_layout: accepted on every chain of ae_cases.REGAE_CASES, refused on the chains this
    route exists for, the LDS bytes compared either way and for both passes."""
    lib = hip.lib()
    chains = [(c.id, A.regae_dims(c)[3], len(c.enc) + 1, True) for c in A.REGAE_CASES]
    chains += [(c.id, G.chain(c), G.n_enc_layers(c), not G.fused_refuses(c)) for c in G.CASES]
    assert sum(not ok for *_, ok in chains) >= 4
    for cid, d, n_enc, ok in chains:
        for with_grad in (0, 1):
            kind, want, *_ = A.mfma_layout(d, bool(with_grad))
            lds = C.c_int64(-1)
            code = lib.cvf_regae_route(_desc(hip, d, n_enc), with_grad, C.byref(lds))
            assert lds.value == want, (cid, with_grad, lds.value, want)
            if want > A.MFMA_LDS_MAX:
                assert code < 0 and f"needs {want} B of LDS" in lib.cvf_last_error().decode(), cid
            else:
                assert code == 1 + (kind == "tight"), (cid, with_grad, code, kind)
        assert (lib.cvf_regae_route(_desc(hip, d, n_enc), 1, None) >= 0) == ok, cid
    for c in A.REGAE_CASES:   # the layout each existing case names is the one the query reports
        assert lib.cvf_regae_route(_desc(hip, A.regae_dims(c)[3], len(c.enc) + 1), 1, None) == 1 + (c.layout == "tight"), c.id
    assert lib.cvf_regae_route(None, 1, None) < 0


def test_workspace_equals_the_mirror(hip):
    lib = hip.lib()
    for c in G.CASES:
        d = G.chain(c)
        for B in (1, c.B, 2 * c.B, 20_000):
            assert lib.cvf_regae_general_scratch_floats(G.mlp_desc(c), B) == G.scratch_floats(d, B) > 0, (c.id, B)
    dip = G.chain(G.CASES[[c.id for c in G.CASES].index("dipeptide-B130")])
    assert dip == [66, 128, 128, 2, 384, 384, 68] and A.n_params(dip) == 200_518 and G.slab_rows(dip, 2 * 313) == 167
    assert 4 * G.scratch_floats(dip, 20_000) < 1 << 30
    cap = G.chain(G.CASES[[c.id for c in G.CASES].index("slab-capped")])
    assert G.slab_rows(cap, 2 * G.n_tiles(G.CAP_B)) == 42 < 2 * G.n_tiles(G.CAP_B) == 46
    assert G.slab_rows([3, 4, 1, 6, 4], 2 * G.n_tiles(G.MANY_B)) == 256 < 2 * G.n_tiles(G.MANY_B) == 258
    assert lib.cvf_regae_general_scratch_floats(G.mlp_desc(G.CASES[0]), 0) == 0
    assert lib.cvf_regae_general_scratch_floats(_desc(hip, [30, 4097, 2, 4097, 31], 2), 100) == 0


@pytest.mark.parametrize("d,K,n_enc,why", [
    ([30, 4097, 2, 4097, 31], 1, 2, "4096 units"),
    ([30, 20, 2, 20, 33], 2, 2, "d_0 = 30 reconstruction rows + K = 2 heads (it has 33 outputs)"),
    ([30, 20, 2, 20, 39], 9, 2, "K = 9"),
    ([30, 20, 2, 20, 31], 1, 1, "the encoder's last layer must have no activation"),
    ([30, 20, 9, 20, 31], 1, 2, "latent width 9 > 8"),
    ([30, 20, 2, 20, 31], 1, 4, "n_enc_layers=4 out of range"),
    ([30, 31], 1, 1, "layers"),
])
def test_refused_chains_say_why(hip, d, K, n_enc, why):
    lib = hip.lib()
    m = _desc(hip, d, 2 if why.startswith("the encoder") else n_enc)
    assert lib.cvf_regae_general_supported(m, K, n_enc) == 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error().decode()
    acts = [m.act[l] for l in range(len(d) - 1)]
    assert not G.supported(d, K, n_enc, acts)
    # the calls themselves refuse the same way, before any launch (no device is touched: this runs without a GPU)
    assert lib.cvf_regae_general_forward(m, None, None, None, 1, 0, 0, K, None, None, None, n_enc, None, None, None) < 0
    assert why in lib.cvf_last_error().decode()
    assert lib.cvf_regae_general_backward(m, None, None, None, 1, 0, 0, K, None, None, 1.0, 1.0, None, None, n_enc, None, None, None,
                                          None, None, None, None) < 0
    assert why in lib.cvf_last_error().decode()


def test_supported_chains(hip):
    lib = hip.lib()
    for c in list(G.CASES) + list(A.REGAE_CASES):
        d, n_enc = A.regae_dims(c)[3], len(c.enc) + 1
        m = _desc(hip, d, n_enc)
        assert lib.cvf_regae_general_supported(m, c.K, n_enc) == 1, (c.id, lib.cvf_last_error())
        assert G.supported(d, c.K, n_enc, [m.act[l] for l in range(len(d) - 1)])
    for act in range(0, 7):
        assert lib.cvf_regae_general_supported(_desc(hip, [30, 4096, 8, 4096, 38], 2, act), 8, 2) == 1
    m = _desc(hip, [30, 20, 2, 20, 31], 2, act=7)
    assert lib.cvf_regae_general_supported(m, 1, 2) == 0 and "activation" in lib.cvf_last_error().decode()
    m = _desc(hip, [30, 20, 2, 20, 31], 2)
    m.n_params += 1
    assert lib.cvf_regae_general_supported(m, 1, 2) == 0 and "outside the chain" in lib.cvf_last_error().decode()
    assert lib.cvf_regae_general_supported(None, 1, 1) == 0
    # good chain, missing buffers
    m = _desc(hip, [30, 20, 2, 20, 31], 2)
    assert lib.cvf_regae_general_forward(m, None, None, None, 1, 0, 0, 1, None, None, None, 2, None, None, None) < 0
    assert "bad argument" in lib.cvf_last_error().decode()


def test_kernels_have_no_scratch_and_fit_the_register_budget(hip, tmp_path):
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "regae_general.o"), tmp_path)
    new = sorted(n for n in kernels if "regaeg_" in n)
    shared = sorted(n for n in kernels if "aeg_" in n and "regaeg_" not in n)
    assert len(new) == 2 and len(shared) == 4 and len(kernels) == 6, sorted(kernels)   # gather, layer, wgrad, loss_sum + out, enc
    for n in new + shared:
        v = kernels[n]
        print(n, v)
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)


def test_the_table_reaches_its_edges(hip):
    lib, cases = hip.lib(), G.CASES
    assert len({c.id for c in cases}) == len(cases) <= 24
    with_grad = [c for c in cases if G.grad(c)]
    merged = {h for c in with_grad for h in G.chain(c)[G.n_enc_layers(c) + 1:-1]}
    assert {1, 31, 32, 33, 63, 64, 65, 130} <= merged
    assert any(c.K == 1 and c.B == 5 for c in with_grad)
    assert any(c.K == G.MAX_NETS and c.k == 3 and c.B == 65 for c in with_grad)
    assert any(c.K == 0 for c in with_grad)
    assert {c.idx for c in with_grad if c.lag_ae == 0 and c.lag_reg > 0} == {True, False}
    assert {c.idx for c in with_grad if (c.lag_ae, c.lag_reg, c.B) == (70, 67, 130)} == {True, False}
    assert any(len(G.chain(c)) - 1 == A.MAX_LAYERS for c in with_grad)
    assert {G.act(c) for c in with_grad} == set(A.ACTS)
    many = [c for c in with_grad if c.B == G.MANY_B]
    assert many and all(c.dup and 2 * G.n_tiles(c.B) > G.MAX_ROWS == G.slab_rows(G.chain(c), 2 * G.n_tiles(c.B)) for c in many)
    capped = [c for c in with_grad if G.slab_rows(G.chain(c), 2 * G.n_tiles(c.B)) < min(2 * G.n_tiles(c.B), G.MAX_ROWS)]
    assert capped
    ids = {c.id: c for c in cases}
    assert ids["dipeptide-B130"].B == 130 and ids["dipeptide-B1001"].B == 1001 and ids["large-molecule-B65"].B == 65
    assert G.chain(ids["dipeptide-B130"])[4] == 384 and ids["large-molecule-B65"].d == 384
    assert sorted(c.B for c in cases if not G.grad(c)) == [1, 1001]
    assert G.FROZEN <= set(ids) and G.ADAM <= {c.id for c in with_grad} and set(G.ACT) <= set(ids)
    for c in cases:
        m = G.mlp_desc(c)
        assert lib.cvf_regae_general_supported(m, c.K, G.n_enc_layers(c)) == 1, (c.id, lib.cvf_last_error())
        assert G.supported(G.chain(c), c.K, G.n_enc_layers(c), G.acts(c))
        refused = lib.cvf_regae_route(m, 1, None) < 0
        assert refused == G.fused_refuses(c) == (c.layout == "refused"), c.id
        if G.grad(c):   # refused by the fused route, or a small shape with its reason - never both, never neither
            assert refused != (c.id in G.SMALL), c.id
    assert set(G.SMALL) <= set(ids) and all(len(why) > 20 for why in G.SMALL.values())


def test_bars_are_tied_to_the_fp32_oracle():
    """Every bar is 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over the table's cases, per term,
    recomputed here from the table's own inputs: between 4 x and 16 x (the rule of ae_cases.REGAE_BARS and its test)."""
    worst = G.group_e32()
    assert set(worst) == set(G.BARS) == set(G.TERMS)
    for term, bar in G.BARS.items():
        assert 4 * worst[term] <= bar <= 16 * worst[term], f"{term}: bar {bar:.2e}, worst e32 {worst[term]:.2e}"


def test_adam_cases_are_ones_the_fp32_oracle_itself_meets():
    import numpy as np
    import torch
    from tests import ae_inputs as I
    from tests.test_ae_sweep_gpu import ADAM_LR, ADAM_STEPS, ADAM_TOL
    assert G.ADAM_SOURCE_MAX == ADAM_TOL / 8 and G.ADAM
    for c in G.CASES:
        if c.id in G.ADAM:
            inp = I.regae_inputs(c)
            p64 = G.oracle(c, inp, torch.float64, ADAM_STEPS, ADAM_LR)[3]
            with G._fixed_order_fp32():
                p32 = G.oracle(c, inp, torch.float32, ADAM_STEPS, ADAM_LR)[3]
            assert float(np.abs(p32 - p64).max()) <= G.ADAM_SOURCE_MAX, c.id
