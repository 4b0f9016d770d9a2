"""CPU (-m "not gpu"): the host-side answers of the CV nets entry (csrc/cv_nets.hip, cvf_cv_nets_*) - the three
symbols in the header, the binding and the library; the models cvf_cv_nets_supported takes and the reasons it gives for the
others; the workspace against the Python mirror of tests/cv_nets_cases.py; the register / scratch budget of the kernels read from
the built code object; where the GPU module's bars come from; and the route ``_CVModel.nets_route()`` reports, from the model
alone."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import codeobj
from tests import cv_nets_cases as N
from tests.test_kernel_resources import kernels_of

NEW = ("cvf_cv_nets_supported", "cvf_cv_nets_scratch_floats", "cvf_cv_nets_eval")


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    codeobj.built_objects()
    return _hip


def _chain(hip, dims, nets=1, act=1):
    """`nets` chains of `dims` over a flat buffer (W then b per layer), `act` after every layer but the last."""
    c = N.Case("x", "A" if nets > 1 else "B", tuple(dims), nets, len(dims) - 1, "tanh", 70, "own", True)
    m = N.mlp_desc(c)
    for l in range(len(dims) - 2):
        m.act[l] = act
    return m


def test_symbols_are_declared_bound_and_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cvf_[a-z0-9_]+)\s*\(", text))
    handle = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip._SIGNATURES and name in hip.EXPORTED_SYMBOLS and hasattr(handle, name), name
        assert hasattr(hip.lib(), name)
    assert set(hip._SIGNATURES) == declared
    # the header names the reference lines the entry serves, and points cvf_mlp_eval_rows' wide chains to it
    header = open(os.path.join(codeobj.ROOT, "include", "cvf.h")).read()
    block = header[header.index("csrc/cv_nets.hip"):header.index("int cvf_cv_nets_supported(")]
    assert "core.py:372-382" in block and "640-647" in block and "855-863" in block
    before = header[header.index("nets forward on row-major features"):header.index("int cvf_mlp_eval_rows(")]
    assert "cvf_cv_nets_eval" in before
    assert os.path.exists(os.path.join(codeobj.CSRC, "cv_nets.hip"))
    assert "cv_nets.hip" in open(os.path.join(codeobj.CSRC, "Makefile")).read()


def test_supported_takes_every_case(hip):
    lib = hip.lib()
    for c in N.CASES:
        assert lib.cvf_cv_nets_supported(N.mlp_desc(c), c.upto, int(c.want_g)) == 1, (c.id, lib.cvf_last_error())
    for act in range(7):   # every activation code, also after the last layer
        m = _chain(hip, [30, 4096, 8], act=act)
        m.act[1] = act
        assert lib.cvf_cv_nets_supported(m, 2, 1) == 1
    assert lib.cvf_cv_nets_supported(_chain(hip, [65536, 4096, 4096], 1), 2, 0) == 1       # the limits themselves
    assert lib.cvf_cv_nets_supported(_chain(hip, [1, 1, 1], 8), 2, 1) == 1
    m = _chain(hip, [30, 20, 2])
    m.n_params += 5                                                                        # offsets may point into a larger buffer
    assert lib.cvf_cv_nets_supported(m, 2, 1) == 1 and lib.cvf_cv_nets_supported(m, 1, 0) == 1


@pytest.mark.parametrize("dims,nets,upto,want_g,why", [
    ([30, 20, 9], 1, 2, 1, "k = 9 outputs"),
    ([30, 4097, 2], 1, 2, 1, "4096 units"),
    ([30] + [4] * 12 + [1], 1, 13, 1, "13 layers"),
    ([30, 20, 2], 3, 2, 1, "must be scalar"),
    ([30, 20, 1], 3, 1, 1, "upto_layer must be 2"),
    ([65537, 20, 1], 1, 2, 1, "65537 input features"),
    ([30, 20, 4097], 1, 2, 0, "4097 outputs"),
    ([30, 20, 2], 1, 3, 1, "upto_layer=3 out of range"),
])
def test_refused_models_say_why(hip, dims, nets, upto, want_g, why):
    lib = hip.lib()
    if len(dims) - 1 > N.MAX_LAYERS:   # (a 13-layer chain does not fit the descriptor: twelve layers' worth of it, n_layers = 13)
        m = _chain(hip, dims[:N.MAX_LAYERS + 1], nets)
        m.n_layers = len(dims) - 1
    else:
        m = _chain(hip, dims, nets)
    assert lib.cvf_cv_nets_supported(m, upto, want_g) == 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error().decode()
    assert lib.cvf_cv_nets_scratch_floats(m, upto, 100, want_g) == 0
    # the call itself refuses the same way, before any launch (no device is touched: this runs without a GPU)
    g = C.c_void_p(64) if want_g else None
    assert lib.cvf_cv_nets_eval(m, None, upto, None, None, 1, None, g, None, None, None) < 0
    assert why in lib.cvf_last_error().decode()


def test_unknown_activation_and_bad_arguments(hip):
    lib = hip.lib()
    m = _chain(hip, [30, 20, 2], act=7)
    assert lib.cvf_cv_nets_supported(m, 2, 1) == 0 and "activation" in lib.cvf_last_error().decode()
    m.act[0], m.act[1] = 1, -1
    assert lib.cvf_cv_nets_supported(m, 2, 1) == 0 and "activation" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_nets_supported(m, 1, 0) == 1          # (the code behind the layers evaluated is not read)
    assert lib.cvf_cv_nets_supported(None, 1, 1) == 0
    # k = 9 is refused only when g is asked for
    m9 = _chain(hip, [30, 20, 9])
    assert lib.cvf_cv_nets_supported(m9, 2, 0) == 1 and lib.cvf_cv_nets_supported(m9, 2, 1) == 0
    # a good model, missing buffers / both inputs
    m = _chain(hip, [30, 20, 2])
    p = C.c_void_p(64)
    assert lib.cvf_cv_nets_eval(m, None, 2, None, None, 1, None, None, None, None, None) < 0
    assert "bad argument" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_nets_eval(m, p, 2, p, p, 1, p, None, None, p, None) < 0
    assert "exactly one" in lib.cvf_last_error().decode()
    assert lib.cvf_cv_nets_eval(m, p, 2, None, None, 1, p, None, None, p, None) < 0
    assert "exactly one" in lib.cvf_last_error().decode()


def test_workspace_equals_the_mirror(hip):
    lib = hip.lib()
    for c in N.CASES:
        m = N.mlp_desc(c)
        for B in (1, c.B, 64, 65, 20_000):
            for want_g in ((0, 1) if c.want_g else (0,)):
                assert lib.cvf_cv_nets_scratch_floats(m, c.upto, B, want_g) == N.scratch_floats(c, B, bool(want_g)) > 0, (c.id, B, want_g)
        assert lib.cvf_cv_nets_scratch_floats(m, c.upto, 0, 0) == 0
    c3 = next(c for c in N.CASES if c.id == "A-config3-k3-B70")
    # config 3 at 20 000 frames: 313 tiles x 64 x (66 + 3 x 61 + 2 x 3 x 20) floats = 29.6 MB
    assert N.scratch_floats(c3, 20_000) == 313 * 64 * (66 + 3 * 61 + 120)


def test_kernels_have_no_scratch_and_fit_the_register_budget(hip, tmp_path):
    kernels = kernels_of(os.path.join(codeobj.built_objects(), "cv_nets.o"), tmp_path)
    own = sorted(n for n in kernels if "cvn_" in n)
    assert len(own) == 2 and any("cvn_layer_kernel" in n for n in own) and any("cvn_linear_kernel" in n for n in own), sorted(kernels)
    assert any("aeg_gather_kernel" in n for n in kernels)
    for n, v in kernels.items():   # every kernel of the object, the copies of csrc/aeg_kernels.hpp included
        print(n, v)
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)


def test_the_table_reaches_its_edges():
    cases = N.CASES
    assert len({c.id for c in cases}) == len(cases)
    A, B = [c for c in cases if c.form == "A"], [c for c in cases if c.form == "B"]
    for dims in ([5, 3, 1], [66, 20, 20, 20, 1], [30, 65, 33, 1], [7, 130, 1], N.DEEP):
        assert {c.nets for c in A if list(c.dims) == dims and c.act == "tanh"} >= {1, 3, 8}, dims
    assert len(N.DEEP) - 1 == N.MAX_LAYERS and N.DEEP[1:-1] == [4] * 11
    assert {c.act for c in A if c.dims == (9, 12, 12, 1)} == set(N.ACTS)
    for dims, upto in (([6, 8, 2], 2), ([30, 65, 33, 3], 3), ([9, 4], 1), ([12, 16, 8], 2), ([64, 4096, 2], 2), ([10, 16, 2, 16, 10], 2)):
        assert any(list(c.dims) == dims and c.upto == upto and c.want_g for c in B), dims
    ae = next(c for c in B if c.layout == "ae")
    assert N.layout(ae)[2] > sum(ae.dims[l + 1] * (ae.dims[l] + 1) for l in range(ae.upto))   # the decoder sits behind the encoder
    assert any(not c.want_g and N.k_of(c) == 100 and list(c.dims) == [20, 32, 100] for c in B)
    for small in ((5, 3, 1), (6, 8, 2)):
        assert sorted(c.B for c in cases if c.dims == small and (c.nets == 3 or c.form == "B")) == sorted(N.EDGE_B)
    assert all(c.B == 70 for c in cases if c.dims not in ((5, 3, 1), (6, 8, 2)))


def test_bars_come_from_the_fp32_evaluation():
    """One bar each for xi and g: BAR_FACTOR = 8 times the worst distance of the fp32 CPU evaluation from the fp64 one over the
    cases - computed, not written down; an fp32 chain's rounding, so between 1e-8 and 1e-4."""
    worst, bars = N.worst_e32(), N.bars()
    assert N.BAR_FACTOR == 8 and set(bars) == {"xi", "g"}
    for term in bars:
        assert bars[term] == 8 * worst[term] and 1e-8 < worst[term] < 1e-4, (term, worst[term])
    print("worst e32", worst, "bars", bars)


def test_nets_route_answers_from_the_model_alone(hip):
    from colvarsfinder import core, nn
    ident = torch.nn.Identity()
    route = lambda nets: core._CVModel(ident, nets).nets_route()
    assert route(nn.EigenFunctions([6, 20, 20, 1], 3)) == ("hip", None)
    assert route(nn.EigenFunctions([6, 12, 1], 1, activation=torch.nn.ELU())) == ("hip", None)
    ae = nn.AutoEncoder([6, 16, 2], [2, 16, 6])
    assert route(ae.encoder) == ("hip", None)
    assert route(nn.create_sequential_nn([6, 4096, 2])) == ("hip", None)
    assert route(torch.nn.Sequential(torch.nn.Linear(6, 4))) == ("hip", None)
    rae = nn.RegAutoEncoder([6, 16, 3], [3, 16, 6], [3, 12, 1], 2)
    assert route(rae.encoder) == ("hip", None)
    for nets, why in ((nn.RegModel(rae, [1, 0]), "RegModel"),
                      (nn.create_sequential_nn([6, 8, 2], activation=torch.nn.GELU()), "GELU"),
                      (nn.EigenFunctions([6, 8, 1], 9), "k = 9"),
                      (nn.create_sequential_nn([6, 8, 9]), "k = 9"),
                      (torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Tanh(), torch.nn.Tanh(), torch.nn.Linear(4, 2)), "child 2"),
                      (torch.nn.Sequential(torch.nn.Linear(6, 4, bias=False)), "bias"),
                      (torch.nn.Linear(6, 2), "Linear")):
        kind, reason = route(nets)
        assert kind == "torch" and why in reason, (kind, reason)
    # a module of the caller's in front: the slow route, whatever the nets are
    from tests.foreign_modules import PairDistances
    kind, reason = core._CVModel(PairDistances(4), nn.EigenFunctions([6, 8, 1], 2)).nets_route()
    assert kind == "torch" and "PairDistances" in reason
    # the plan reads the modules every time: a replaced weight is the one the next call gathers
    cv = core._CVModel(ident, ae.encoder)
    p0 = torch.cat([p.reshape(-1) for p in cv._nets_plan(ae.encoder)[3]])
    with torch.no_grad():
        ae.encoder[0].weight.add_(1.0)
    p1 = torch.cat([p.reshape(-1) for p in cv._nets_plan(ae.encoder)[3]])
    assert not torch.equal(p0, p1)
