"""CPU: every compiled instance of the autoencoder step's kernels (csrc/ae.hip: ae16_kernel<RTD, RTH>, ae_mfma_kernel<TANH>) is
claimed by a case of the GPU sweep (tests/ae_cases.py, run by tests/test_ae_sweep_gpu.py) or listed as unreachable with a reason;
the table reaches the edges it was built for; its mirror of the host's decisions agrees with the library; and its error bars
stay tied to the fp32 oracle they were derived from.

The instances are read from the built code object, so a new AE16_CASE in ae16_dispatch, or a case dropped from the table,
turns this module red and names what no case reaches.
"""
import ctypes as C
import os

import pytest

from tests import ae_cases as A
from tests.codeobj import built_objects, kernels_of, template_args

FAMILIES = [("ae16_kernel", 2), ("ae_mfma_kernel", 1)]   # (kernel template, template arguments of the instance key)
AE16 = [c for c in A.CASES if A.route(c) == "ae16"]
MFMA = [c for c in A.CASES if A.route(c) in ("mfma_tanh", "mfma_any")]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    names = kernels_of(os.path.join(built_objects(), "ae.o"), tmp_path_factory.mktemp("ae_o"))
    out = set()
    for family, n in FAMILIES:
        keys = {template_args(name, family) for name in names} - {None}
        assert keys, f"no {family} instance in ae.o"
        out |= {(family,) + key[:n] for key in keys}
    return out


def _names(instances):
    return ", ".join(f"{f}<{', '.join(map(str, a))}>" for f, *a in sorted(instances))


def test_every_compiled_ae_instance_is_claimed_by_a_case(compiled):
    missing = compiled - A.claimed() - set(A.UNREACHABLE)
    assert not missing, "kernel instances no case of tests/ae_cases.py launches (add a case, or list it in UNREACHABLE with the " \
                        "reason): " + _names(missing)


def test_cases_claim_only_compiled_instances(compiled):
    stale = (A.claimed() | set(A.UNREACHABLE)) - compiled
    assert not stale, "instances the table claims but ae.o does not hold: " + _names(stale)
    assert all(isinstance(reason, str) and reason for reason in A.UNREACHABLE.values())


def test_instance_counts(compiled):
    """ae16_dispatch: RTD 1..5 x RTH 1..2; ae_mfma_kernel: tanh inlined, and the run-time activation switch."""
    count = {f: sum(1 for i in compiled if i[0] == f) for f, _ in FAMILIES}
    assert count == {"ae16_kernel": 10, "ae_mfma_kernel": 2}
    assert {i[1:] for i in A.claimed() if i[0] == "ae16_kernel"} == set(A.AE16_INSTANCES)


def test_case_ids_and_flags_are_consistent():
    ids = [c.id for c in A.CASES]
    assert len(set(ids)) == len(ids)
    for c in A.CASES:
        assert c.e_dims[-1] == c.d_dims[0] and c.e_dims[0] == c.d_dims[-1] and len(c.e_dims) >= 2 and len(c.d_dims) >= 2, c
        assert len(A.dims(c)) - 1 <= A.MAX_LAYERS and c.B >= 1 and c.act in A.ACTS, c
        assert c.grad or not c.adam, c                             # Adam needs the gradient
        group = c.id.split("-")[0] + "-" + c.id.split("-")[1]
        if group == "ae16-inst" or (group == "ae16-edge" and "over-80k" not in c.id):
            assert A.route(c) == "ae16", (c.id, A.route(c))
        if group == "mfma-tanh":
            assert A.route(c) == ("refused" if "refused" in c.id else "mfma_tanh"), c.id
        if group == "mfma-any":
            assert A.route(c) == "mfma_any", c.id
        if A.route(c) != "refused":
            assert A.group(c) in A.BARS, c.id
    assert sum(A.route(c) == "refused" for c in A.CASES) <= 2      # the only cases without a value comparison


def test_ae16_case_count_per_instance():
    """A case dropped from the table shows up here with the instance it covered (a deliberate change updates the figures)."""
    count = {}
    for c in AE16:
        inst = A.ae16_instance(A.dims(c))
        count[inst] = count.get(inst, 0) + 1
    assert count == {(1, 1): 9, (1, 2): 2, (2, 1): 4, (2, 2): 7, (3, 1): 3, (3, 2): 3, (4, 1): 2, (4, 2): 2, (5, 1): 3, (5, 2): 9}


def test_ae16_cases_reach_the_edges():
    for inst in A.AE16_INSTANCES:
        mine = [c for c in AE16 if A.ae16_instance(A.dims(c)) == inst]
        assert any(any(d % 4 for d in A.dims(c)) for c in mine), f"{inst}: no width off a multiple of 4"
        assert any(c.B % A.TILE for c in mine), f"{inst}: no ragged last tile"
        assert any(c.grad for c in mine), inst
    assert {1, 2, 16, 17, 77, 80} <= {c.e_dims[0] for c in AE16}
    hidden = set().union(*[set(A.dims(c)[1:-1]) for c in AE16])
    assert {1, 31, 32} <= hidden
    assert any(c.e_dims[-1] == 1 for c in AE16)                     # a 1-wide latent
    depths = {len(A.dims(c)) - 1 for c in AE16}
    assert 2 in depths and A.MAX_LAYERS in depths
    lds = [A.ae16_lds_bytes(A.dims(c)) for c in AE16]
    assert max(lds) <= A.AE16_LDS_MAX and any(v > A.OPT_IN_LDS for v in lds) and any(v <= A.OPT_IN_LDS for v in lds)
    assert any(A.AE16_LDS_MAX - 4096 <= v for v in lds)            # within 4 KiB under the line
    # ... and an ae16 shape in every other respect just above it, where the route must flip
    over = [c for c in A.CASES if A.route(c) == "mfma_tanh" and not c.no_ae16 and not c.misaligned
            and A.ae16_instance(A.dims(c)) and A.AE16_LDS_MAX < A.ae16_lds_bytes(A.dims(c)) <= A.AE16_LDS_MAX + 4096]
    assert over and all(not A.ae16_shape(A.dims(c), c.act) for c in over)
    assert {1, 5, 63, 64, 65, 130} <= {c.B for c in AE16}
    big = [c for c in AE16 if c.B > A.MAX_BLOCKS * A.TILE]
    assert all(c.dup for c in A.CASES if c.B > A.MAX_BLOCKS * A.TILE)     # every batch above 2048 tiles also as two copies
    assert any(A.grid(c.B)[1] == 2 and c.B % A.TILE and c.grad for c in big)
    assert {c.idx for c in AE16} == {True, False} and {c.idx for c in big} == {True, False}
    assert {c.grad for c in AE16} == {True, False}


def test_mfma_cases_reach_the_edges():
    seen = {(A.route(c), A.mfma_layout(A.dims(c), c.grad)[0], c.grad) for c in MFMA}
    assert seen == {(r, lay, g) for r in ("mfma_tanh", "mfma_any") for lay in ("roomy", "tight") for g in (True, False)}
    for c in MFMA:
        name, lds, skip0, tail = A.mfma_layout(A.dims(c), c.grad)
        assert (skip0 > 0) == (name == "tight") and lds <= A.MFMA_LDS_MAX, c.id
    for r in ("mfma_tanh", "mfma_any"):
        lds = [A.lds_bytes(c) for c in MFMA if A.route(c) == r]
        assert min(lds) <= A.OPT_IN_LDS < max(lds), r
        assert any(A.mfma_layout(A.dims(c), c.grad)[3] for c in MFMA if A.route(c) == r), f"{r}: no theta shorter than 32 AP floats"
        assert any(c.B % A.TILE == 0 for c in MFMA if A.route(c) == r) and any(c.B % A.TILE for c in MFMA if A.route(c) == r)
        assert any(A.grid(c.B)[1] > 1 for c in MFMA if A.route(c) == r)
    assert any(c.misaligned for c in MFMA) and any(c.no_ae16 for c in MFMA)
    assert all(A.ae16_shape(A.dims(c), c.act) for c in MFMA if c.misaligned or c.no_ae16)   # they fall back, nothing else does it
    refused = [c for c in A.CASES if A.route(c) == "refused"]
    assert refused and all(A.MFMA_LDS_MAX < A.lds_bytes(c) <= A.MFMA_LDS_MAX + 4096 for c in refused)   # just over 160 KiB
    assert set(A.ACTS) == {c.act for c in A.CASES}
    assert sum(c.dup for c in A.CASES) >= 4 and {A.route(c) for c in A.CASES if c.adam} >= {"ae16", "mfma_tanh", "mfma_any"}
    adam = [c for c in A.CASES if c.adam]
    assert {A.ae16_instance(A.dims(c))[1] for c in adam if A.route(c) == "ae16"} == {1, 2}
    assert {A.mfma_layout(A.dims(c), True)[0] for c in adam if A.route(c) != "ae16"} == {"roomy", "tight"}


def test_known_layout_sizes():
    """Figures quoted in csrc/ae.hip and DESIGN.md, recomputed by the mirror."""
    config2 = [66, 20, 20, 20, 2, 10, 10, 66]
    assert A.ae16_lds_bytes(config2) == 78_848 and A.ae16_instance(config2) == (5, 2)
    wide = [80, 32, 32, 3, 32, 32, 80]
    assert A.ae16_lds_bytes(wide) == 126_976 and not A.ae16_shape(wide, "tanh")
    assert A._mfma_layout_of(wide, True, False)[0] * 4 == 97_744 and A._mfma_layout_of(wide, True, True)[0] * 4 == 87_504
    assert A.mfma_layout(wide, True)[0] == "roomy"
    for rtd, rth in A.AE16_INSTANCES:
        d0, h = 16 * rtd - 3, 16 * rth - 5
        assert 21_760 <= A.ae16_lds_bytes([d0, h, 2, h, d0]) <= 72_128
    assert A.grid(A.BIG_B) == (2048, 2) and A.grid(20_000) == (313, 1) and A.grid(1) == (1, 1)


def test_mirror_agrees_with_the_library(monkeypatch):
    """cvf_ae_step_route and cvf_ae_scratch_floats are host arithmetic: the library answers them without a GPU."""
    from colvarsfinder import _hip
    from tests import ae_inputs as I
    built_objects()
    lib = _hip.lib()
    for c in A.CASES:
        if c.no_ae16:
            monkeypatch.setenv("CVF_NO_AE16", "1")
        else:
            monkeypatch.delenv("CVF_NO_AE16", raising=False)
        lds, d = C.c_int64(-1), I.mlp_desc(c)
        code = lib.cvf_ae_step_route(d, C.c_void_p(4096 + 4 * c.misaligned), int(c.grad), C.byref(lds))
        assert (code, lds.value) == (A.route_code(c), A.lds_bytes(c)), c.id
        if code < 0:
            assert f"{A.lds_bytes(c)} B of LDS" in lib.cvf_last_error().decode()
        for B in (c.B, 2 * c.B):
            assert lib.cvf_ae_scratch_floats(d, B) == A.scratch_floats(A.dims(c), B), (c.id, B)


def test_bars_are_tied_to_the_fp32_oracle():
    """Every bar is 8 x the worst distance of the fp32 CPU oracle from the fp64 oracle over its group's cases, as recomputed here
    from the table's own inputs: between 4 x and 16 x, so that the bars can neither drift from their source nor flake on the
    last digit of an fp32 sum."""
    from tests import ae_inputs as I
    worst = I.group_e32()
    assert set(worst) == set(A.BARS)
    for g, bars in A.BARS.items():
        for what, bar, e in zip(("loss", "gradient"), bars, worst[g]):
            assert 4 * e <= bar <= 16 * e, f"{g} {what}: bar {bar:.2e}, worst e32 {e:.2e}"


def test_regae_table_reaches_its_edges_and_its_bars_are_tied_to_the_fp32_oracle():
    from tests import ae_inputs as I
    R = A.REGAE_CASES
    assert len({c.id for c in R}) == len(R) <= 14
    assert {c.K for c in R} == {1, 4, 8} and {5, 63, 65, 130} <= {c.B for c in R} and {c.idx for c in R} == {True, False}
    assert any(c.lag_ae == 0 for c in R) and any(c.lag_ae >= A.TILE and c.lag_reg >= A.TILE for c in R)   # partners in another tile
    for c in R:
        chain = A.regae_dims(c)[3]
        assert A.mfma_layout(chain, True)[0] == c.layout and len(chain) - 1 <= A.MAX_LAYERS and c.lag_reg >= 1, c.id
    assert {c.layout for c in R} == {"roomy", "tight"} and sum(c.handoff for c in R) >= 2
    big = [c for c in R if c.dup]
    assert big and all(c.B > 65_536 and A.regae_grid(c) == (A.MAX_BLOCKS, 2) and c.B % A.TILE for c in big)
    worst = I.regae_group_e32()
    for term in A.REGAE_TERMS:
        assert 4 * worst[term] <= A.REGAE_BARS[term] <= 16 * worst[term], f"{term}: bar {A.REGAE_BARS[term]:.2e}, worst e32 {worst[term]:.2e}"
