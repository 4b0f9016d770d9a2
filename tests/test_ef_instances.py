"""CPU: every compiled instance of the eigenfunction step's kernels is claimed by a case of the GPU sweep (tests/ef_cases.py,
run by tests/test_ef_sweep_gpu.py) or listed as unreachable with a reason.

The instances are read from the built code objects, so a new (H, NH) in ef16_dispatch / ef_dispatch, a new NIT, or a case
dropped from the table turns this test red and names what no case reaches.
"""
import os

import pytest

from tests import ef_cases as E
from tests.codeobj import built_objects, kernels_of, template_args

# (object file, kernel template, number of template arguments that make up the instance key)
FAMILIES = [("ef16_front.o", "ef16_front_kernel", 4), ("ef16_back.o", "ef16_back_kernel", 4),
            ("ef_mfma.o", "ef_bwd_mfma_kernel", 2), ("ef_mfma.o", "ef_fwd_metric_kernel", 2), ("ef_mfma.o", "ef_align_fwd_kernel", 2)]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{instance key as in ef_cases.instances()} of the five families in the built objects."""
    built = built_objects()
    out, objs = set(), {}
    for obj, family, n in FAMILIES:
        if obj not in objs:
            objs[obj] = kernels_of(os.path.join(built, obj), tmp_path_factory.mktemp(obj.replace(".", "_")))
        keys = {template_args(name, family) for name in objs[obj]} - {None}
        assert keys, f"no {family} instance in {obj}"
        out |= {(family,) + key[:n] for key in keys}
    return out


def test_every_compiled_step_instance_is_claimed_by_a_case(compiled):
    missing = compiled - E.claimed() - set(E.UNREACHABLE)
    assert not missing, "kernel instances no case of tests/ef_cases.py launches (add a case, or list it in UNREACHABLE with the " \
                        "reason): " + ", ".join(f"{f}<{', '.join(map(str, a))}>" for f, *a in sorted(missing))


def test_cases_claim_only_compiled_instances(compiled):
    """The table's mirror of the dispatch names instances that exist (a stale rule would claim coverage of nothing)."""
    stale = (E.claimed() | set(E.UNREACHABLE)) - compiled
    assert not stale, f"instances the table claims but the objects do not hold: {sorted(stale)}"


def test_instance_counts():
    """16 (H, NH) x (NIT 1..6 x ALLAL + the transfer instance) front and 16 x MULTI x GEN back instances."""
    c = E.claimed()
    count = {f: sum(1 for i in c if i[0] == f) for _, f, _ in FAMILIES}
    assert count == {"ef16_front_kernel": 16 * 13, "ef16_back_kernel": 16 * 4, "ef_bwd_mfma_kernel": 24,
                     "ef_fwd_metric_kernel": 20, "ef_align_fwd_kernel": 20}


def test_each_case_takes_the_route_its_group_is_for():
    for c in E.CASES:
        group = c.id.split("-")[1]
        want = {"ef16": "ef16", "multi": "ef16", "mixed": "plain", "fused": "fused"}[group]
        assert E.route(c) == want, (c, E.route(c))
        assert c.layout == "mixed" or 3 <= c.n_align <= c.n_rec <= c.n_atoms, c
        assert 1 <= c.k <= E.MAX_NETS and c.B >= 1, c
        if c.dup:   # the half batch is not MULTI, the doubled one is
            (back,) = [i for i in E.instances(c) if i[0] == "ef16_back_kernel"]
            (back2,) = [i for i in E.instances(c, 2 * c.B) if i[0] == "ef16_back_kernel"]
            assert back[3] == 0 and back2[3] == 1, c


def test_generator_sweep_reaches_the_edges():
    """Ragged and full last iterations, strict-prefix alignment, trailing frame atoms, k 1..8, ragged tiles and, for every
    (H, NH), a front launch above 48 KiB of LDS (the hipFuncSetAttribute branch, ef16_front.hip:720)."""
    gen = [c for c in E.CASES if c.id.startswith("gen-ef16-")]
    assert len(gen) == len(E.EF16_SHAPES) * 12
    for nit in range(1, 7):
        rec = {c.n_rec % 4 for c in gen if (c.n_rec + 3) // 4 == nit}
        assert 0 in rec and rec - {0}, (nit, rec)
    assert any(c.n_align < c.n_rec for c in gen) and any(c.n_atoms > c.n_rec for c in gen)
    assert {c.k for c in gen} == set(range(1, E.MAX_NETS + 1))
    assert all(c.B % 64 for c in gen)
    for H, NH in E.EF16_SHAPES:
        lds = [E.front16_lds_bytes(3 * c.n_atoms, c.n_align, c.k) for c in gen if E.shape(c) == (H, NH)]
        assert max(lds) > 48 * 1024, (H, NH, max(lds))
