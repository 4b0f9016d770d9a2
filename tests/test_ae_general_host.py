"""CPU (-m "not gpu"): the per-layer autoencoder route's host-side answers (csrc/ae_general.hip) - the chains it takes and the
reasons it gives for the others, its workspace against the Python mirror of tests/ae_general_cases.py and the bound DESIGN.md
section 4.10 states, its three C entries in the header, the binding and the library, the register / scratch budget of its
kernels read from the built code object, and the case table of the GPU module: what it reaches and where its bars come from."""
import ctypes as C
import os
import re

import pytest

from tests import ae_cases as A
from tests import ae_general_cases as G
from tests import codeobj

GIB = 1 << 30
NEW = ("cvf_ae_general_supported", "cvf_ae_general_scratch_floats", "cvf_ae_general_step")


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _desc(hip, d, act=1, last_act=0):
    """One chain over a flat buffer in parameters() order; `act` after every layer but the last."""
    m, L, pos = hip.MLPDesc(), len(d) - 1, 0
    m.n_nets, m.n_layers = 1, L
    for l in range(L):
        m.dims[l], m.dims[l + 1], m.act[l] = d[l], d[l + 1], (act if l < L - 1 else last_act)
        m.w_off[0][l], pos = pos, pos + d[l] * d[l + 1]
        m.b_off[0][l], pos = pos, pos + d[l + 1]
    m.n_params = pos
    return m


SUPPORTED = [[384, 256, 64, 2, 64, 256, 384], [66, 128, 128, 2, 128, 128, 66], [120, 56, 24, 3, 24, 56, 120], [3, 3], [1, 1, 1],
             [30, 4096, 30], [65536, 1, 65536], [65536, 4032, 2, 65536], [30, 17, 13, 9, 5, 3, 2, 3, 5, 9, 13, 17, 30]]


@pytest.mark.parametrize("d", SUPPORTED, ids=["x".join(map(str, d[:3])) + f"-L{len(d) - 1}" for d in SUPPORTED])
def test_supported_shapes(hip, d):
    for act in range(0, 7):
        assert hip.lib().cvf_ae_general_supported(_desc(hip, d, act)) == 1, hip.lib().cvf_last_error()
    assert G.supported(d)
    assert hip.lib().cvf_ae_general_scratch_floats(_desc(hip, d), 100) == G.scratch_floats(d, 100)


@pytest.mark.parametrize("d,why", [([30, 4097, 30], "4096 units"), ([30, 20, 31], "output width 31 != input width 30"),
                                   ([65537, 2, 65537], "input features"), ([30, 0, 30], "1 to 4096 units"),
                                   # 64 x 1025 and 1024 x 65 blocks of 64 x 64 weights: past a launch's grid.y
                                   ([65536, 4096, 65536], "more than 65535 blocks"), ([65536, 4033, 2, 65536], "more than 65535 blocks")])
def test_refused_widths_say_why(hip, d, why):
    m = _desc(hip, d)
    assert hip.lib().cvf_ae_general_supported(m) == 0 and not G.supported(d)
    assert why in hip.lib().cvf_last_error().decode()
    assert hip.lib().cvf_ae_general_scratch_floats(m, 100) == 0


def test_refused_descriptions_say_why(hip):
    lib, good = hip.lib(), [30, 20, 2, 20, 30]
    m = _desc(hip, good)
    m.n_nets = 2
    assert lib.cvf_ae_general_supported(m) == 0 and "one chain" in lib.cvf_last_error().decode()
    m = _desc(hip, good)
    m.n_layers = 13   # past what the descriptor can describe
    assert lib.cvf_ae_general_supported(m) == 0 and "1 to 12" in lib.cvf_last_error().decode()
    m = _desc(hip, good)
    m.n_layers = 0
    assert lib.cvf_ae_general_supported(m) == 0 and "layers" in lib.cvf_last_error().decode()
    m = _desc(hip, good, act=7)
    assert lib.cvf_ae_general_supported(m) == 0 and "activation" in lib.cvf_last_error().decode()
    m = _desc(hip, good)
    m.n_params += 1   # parameters no layer owns: their slab entries would never be written
    assert lib.cvf_ae_general_supported(m) == 0 and "outside the chain" in lib.cvf_last_error().decode()
    m = _desc(hip, good)
    m.b_off[0][3] = m.n_params - 1
    assert lib.cvf_ae_general_supported(m) == 0 and "outside the flat buffer" in lib.cvf_last_error().decode()
    assert lib.cvf_ae_general_supported(None) == 0
    assert lib.cvf_ae_general_scratch_floats(_desc(hip, good), 0) == 0
    # the step itself refuses the same way, before any launch (no device is touched: this runs without a GPU)
    m = _desc(hip, [30, 4097, 30])
    assert lib.cvf_ae_general_step(m, None, None, None, 1, None, 1.0, None, None, None, None, None, None) < 0
    assert "4096 units" in lib.cvf_last_error().decode()
    assert lib.cvf_ae_general_step(_desc(hip, good), None, None, None, 1, None, 1.0, None, None, None, None, None, None) < 0
    assert "bad argument" in lib.cvf_last_error().decode()


def test_workspace_equals_the_mirror_and_stays_under_a_gib(hip):
    lib = hip.lib()
    from tests import ae_inputs as I
    for c in G.CASES:
        d = G.dims(c)
        for B in (1, c.B, 2 * c.B, 20_000):
            assert lib.cvf_ae_general_scratch_floats(I.mlp_desc(c), B) == G.scratch_floats(d, B), (c.id, B)
    big = G.BIG_E + G.BIG_D[1:]
    assert A.n_params(big) == 230_658 and G.slab_rows(big, 20_000) == 145          # (128 MiB / 922 632 B)
    need = lib.cvf_ae_general_scratch_floats(_desc(hip, big), 20_000)
    assert need == G.scratch_floats(big, 20_000) and 4 * need < GIB, need
    # slab rows: never more than tiles, 256 or what 128 MiB holds, and at least one
    assert G.slab_rows([3, 5, 3], 130) == 3 and G.slab_rows([3, 5, 3], G.MANY_B) == 256
    cap = G.CAP_E + G.CAP_D[1:]
    assert A.n_params(cap) == 131_966 > 131_072 and G.slab_rows(cap, G.CAP_B) == 254 and G.n_tiles(G.CAP_B) == 256
    assert 4 * 254 * A.n_params(cap) <= G.SLAB_BYTES < 4 * 255 * A.n_params(cap)
    wide = [4096, 4096, 4096, 4096]                                                  # one row is larger than the budget
    assert 4 * A.n_params(wide) > G.SLAB_BYTES and G.slab_rows(wide, 20_000) == 1
    assert lib.cvf_ae_general_scratch_floats(_desc(hip, wide), 20_000) == G.scratch_floats(wide, 20_000)


def test_header_binding_and_exports_agree(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and hasattr(handle, name), name
    assert set(hip._SIGNATURES) == declared                                          # binding <-> header, both directions
    # the step takes cvf_ae_step's exact argument list
    assert hip._SIGNATURES["cvf_ae_general_step"][0] is hip._SIGNATURES["cvf_ae_step"][0]
    assert list(hip._SIGNATURES["cvf_ae_general_step"][1]) == list(hip._SIGNATURES["cvf_ae_step"][1])
    arglist = lambda name: re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)).strip()
    assert arglist("cvf_ae_general_step") == arglist("cvf_ae_step")
    assert os.path.exists(os.path.join(codeobj.CSRC, "ae_general.hip"))


def test_kernels_have_no_scratch_and_fit_the_register_budget(hip, tmp_path):
    kernels = codeobj.kernels_of(os.path.join(codeobj.built_objects(), "ae_general.o"), tmp_path)
    names = sorted(n for n in kernels if "aeg_" in n)
    assert len(names) == 5 and len(kernels) == 5, sorted(kernels)
    assert not any("efg_" in n for n in kernels)
    for n in names:
        v = kernels[n]
        print(n, v)
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
        # (256-thread blocks, at most 128 VGPRs - four waves per SIMD)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)


def test_the_table_reaches_its_edges(hip):
    from tests import ae_inputs as I
    lib, cases = hip.lib(), G.CASES
    assert len({c.id for c in cases}) == len(cases) <= 40
    hidden = {h for c in cases if c.grad for h in G.dims(c)[1:-1]}
    assert {1, 31, 32, 33, 63, 64, 65, 130} <= hidden
    assert {1, 3, 67, 384} <= {c.e_dims[0] for c in cases if c.grad}
    assert {1, 63, 64, 65, 130, 257} <= {c.B for c in cases if c.grad}
    assert {len(G.dims(c)) - 1 for c in cases} >= {2, A.MAX_LAYERS}
    assert {c.act for c in cases if c.grad} == set(A.ACTS)
    assert {c.idx for c in cases if c.grad} == {True, False} == {c.idx for c in cases if not c.grad}
    assert any(c.misaligned and c.grad for c in cases) and sum(not c.grad for c in cases) >= 2
    assert sum(c.adam for c in cases) == 2 and sum(c.dup for c in cases) == 1
    many = [c for c in cases if c.B == G.MANY_B]
    assert many and all(G.n_tiles(c.B) == G.slab_rows(G.dims(c), c.B) + 1 == 257 for c in many)
    capped = [c for c in cases if G.slab_rows(G.dims(c), c.B) < min(G.n_tiles(c.B), G.MAX_ROWS)]
    assert capped and all(c.grad and G.n_tiles(c.B) > G.slab_rows(G.dims(c), c.B) for c in capped)
    assert any(list(c.e_dims) == G.BIG_E and list(c.d_dims) == G.BIG_D and c.B == 130 and c.grad for c in cases)
    for c in cases:
        m = I.mlp_desc(c)
        assert G.supported(G.dims(c)) and lib.cvf_ae_general_supported(m) == 1, c.id
        if c.grad:   # refused by the fused step, or a small shape with its reason - never both, never neither
            refused = lib.cvf_ae_step_route(m, C.c_void_p(4096 + 4 * c.misaligned), 1, None) < 0
            assert refused == (A.route(c) == "refused") and refused != (c.id in G.SMALL), c.id
    assert set(G.SMALL) <= {c.id for c in cases} and all(len(why) > 20 for why in G.SMALL.values())


def test_bars_are_tied_to_the_fp32_oracle():
    """Every bar is 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over its group's cases, recomputed here
    from the table's own inputs: between 4 x and 16 x (the rule of ae_cases.BARS and its test)."""
    worst = G.group_e32()
    assert set(worst) == set(G.BARS) == {G.group(c) for c in G.CASES}
    for g, bars in G.BARS.items():
        for what, bar, e in zip(("loss", "gradient"), bars, worst[g]):
            assert 4 * e <= bar <= 16 * e, f"{g} {what}: bar {bar:.2e}, worst e32 {e:.2e}"


def test_adam_cases_are_ones_the_fp32_oracle_itself_meets():
    """Three Adam steps amplify the rounding of gradient entries next to zero in any fp32 evaluation; the cases held to
    ADAM_TOL are those on which torch's own fp32 steps on the CPU stay within an eighth of it (ae_general_cases.ADAM_SOURCE_MAX)."""
    import numpy as np
    import torch
    from tests import ae_inputs as I
    from tests.test_ae_sweep_gpu import ADAM_LR, ADAM_STEPS, ADAM_TOL
    assert G.ADAM_SOURCE_MAX == ADAM_TOL / 8
    for c in G.CASES:
        if c.adam:
            inp = I.inputs(c)
            p64, p32 = (I.oracle(c, inp, dt, ADAM_STEPS, ADAM_LR)[2] for dt in (torch.float64, torch.float32))
            assert float(np.abs(p32 - p64).max()) <= G.ADAM_SOURCE_MAX, c.id
