"""GPU (-m gpu): ``cvf_align_feature_vjp``, ``_vjp_rows``, ``_jvp`` and ``_hvp`` on every compiled instance of their kernels, through
the C ABI, against the fp64 oracle - the table of tests/align_deriv_cases.py (its docstring: reference, error measure, bars).

Each (case, entry point) calls ``cvf_align_feature_fwd`` for the aux rows, asserts the instance ``cvf_align_feature_deriv_route`` names
for the very pointers of the call - the function the launch decides by - and then holds the result to the per-frame, per-type bars.
Every output starts as NaN: an element left unwritten fails.  A repeated call must give the same bits; ``vjp_rows`` must equal k
single calls bit for bit (on the grouped and the multi-launch cases too); a call whose output row lies 4 bytes past a 16-byte
boundary must equal the aligned call bit for bit; atoms nothing reads come out exactly 0, and NaN tangents there reach nothing.
The layers without alignment also run ``cvf_align_feature_fwd`` and ``cvf_metric_apply`` at every frames-per-workgroup step.
With CVF_SWEEP_ERRORS set the module adds its {case: {quantity: error}} table through tests/sweep_errors.py."""
import numpy as np
import pytest
import torch

from tests import align_deriv_cases as D
from tests import sweep_errors
from tests.align_hvp_cases import frame_errors

pytestmark = pytest.mark.gpu

ERRORS = {}      # case id -> {"run/type": error / bar ...}; written to $CVF_SWEEP_ERRORS when set
_PREPARED = {}   # case id -> abi_prepare(case): one forward call per case, shared by its entry points


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    _PREPARED.clear()
    sweep_errors.write(ERRORS)


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def prepared(case, dev):
    if case.id not in _PREPARED:
        _PREPARED[case.id] = D.abi_prepare(case, dev)
    return _PREPARED[case.id]


def route(p, run, aligned16=True):
    """The plan of the call, asserted against the mirrors: a case that silently changes instance fails here."""
    rc, plan = D.abi_route(p.desc, p.B, D.WHICH[run], p.case.k, aligned16)
    want = D.expected_plan(p.case, D.WHICH[run], aligned16=aligned16)
    assert rc == 0 and plan == want, (p.case.id, run, plan, want)
    return plan


def held(case, run, t, got, want, bar):
    """The per-frame error of one type against its bar (recorded, printed, asserted)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), f"{case.id} {run}/{t}: an element was not written"
    if not np.abs(want).any():
        assert not got.any(), f"{case.id} {run}/{t}: must be exactly 0"
        err = 0.0
    else:
        err = float(frame_errors(got, want).max())
    ERRORS.setdefault(case.id, {})[f"{run}/{t}"] = err
    ERRORS[case.id][f"{run}/{t}/bar"] = bar
    print(f"[deriv] {case.id:20s} {run:6s} {t:9s} B {case.B:3d} err {err:.2e} bar {bar:.2e} ({err / bar:.2f})", flush=True)
    assert bar <= D.CEILING and err <= bar, (case.id, run, t, err, bar)
    return err


def unread_is_zero(p, out):
    assert p.s.unused and not out.reshape(p.B, -1, p.case.n, 3)[:, :, p.s.unused].any(), f"{p.case.id}: an atom nothing reads is not 0"


def check_vjp(p, ref):
    case, s = p.case, p.s
    plan = route(p, "vjp")
    outs = {}
    for t in [D.DENSE] + list(s.cols):
        outs[t] = D.abi_vjp(p, D.cotangent(s, t))
        held(case, "vjp", t, outs[t], ref.ref["vjp"][t], ref.bar["vjp"][t])
        unread_is_zero(p, outs[t])
    assert D.same_bits(outs[D.DENSE], D.abi_vjp(p, s.g)), f"{case.id}: a repeated call gives other bits"
    if case.id in D.MISALIGNED:
        off = route(p, "vjp", aligned16=False)
        assert plan["vec4"] == 1 and off["vec4"] == 0
        assert D.same_bits(outs[D.DENSE], D.abi_vjp(p, s.g, misaligned=True)), f"{case.id}: the scalar stores give other bits"


def check_rows(p, ref):
    case, s, k = p.case, p.s, p.case.k
    plan = route(p, "rows")
    kinds = [D.DENSE] + list(s.cols)
    G = [D.cotangent(s, t).float() for t in kinds]
    single = [D.abi_vjp(p, g) for g in G]
    first = None
    for start in range(0, len(kinds), k):                  # row i of a call: cotangent (start + i) mod 5, so every type is a row of some call
        idx = [(start + i) % len(kinds) for i in range(k)]
        g_rows = torch.stack([G[j] for j in idx], dim=1)
        out = D.abi_rows(p, g_rows)
        first = (g_rows, out) if first is None else first
        unread_is_zero(p, out)
        for i, j in enumerate(idx):
            assert D.same_bits(out[:, i], single[j]), f"{case.id}: row {i} of vjp_rows (rows per pass {plan['rows_per_launch']}, " \
                f"launches {plan['launches']}) differs from the single call"
            held(case, "rows", kinds[j], out[:, i], ref.ref["vjp"][kinds[j]], ref.bar["vjp"][kinds[j]])
    assert D.same_bits(first[1], D.abi_rows(p, first[0])), f"{case.id}: a repeated call gives other bits"
    if case.id in D.MISALIGNED:
        off = route(p, "rows", aligned16=False)
        assert plan["vec4"] == 1 and off["vec4"] == 0 and off["launches"] == plan["launches"] > 1
        assert D.same_bits(first[1], D.abi_rows(p, first[0], misaligned=True)), f"{case.id}: the scalar stores give other bits"


def check_jvp(p, ref):
    case, s = p.case, p.s
    route(p, "jvp")
    q = D.abi_jvp(p, s.u)
    assert q.shape == ref.ref["jvp"].shape and np.isfinite(q).all(), f"{case.id}: q not fully written"
    for t, c in s.cols.items():
        held(case, "jvp", t, q[:, c], ref.ref["jvp"][:, c], ref.bar["jvp"][t])
    assert D.same_bits(q, D.abi_jvp(p, s.u)), f"{case.id}: a repeated call gives other bits"
    nan = s.u.clone()
    nan[:, s.unused] = float("nan")
    assert s.unused and D.same_bits(q, D.abi_jvp(p, nan)), f"{case.id}: the tangent of an atom nothing reads reaches q"


def check_hvp(p, ref):
    case, s = p.case, p.s
    plan = route(p, "hvp")
    outs = {}
    for t in [D.DENSE] + list(s.cols):
        outs[t] = D.abi_hvp(p, D.cotangent(s, t), s.u)
        held(case, "hvp", t, outs[t], ref.ref["hvp"][t], ref.bar["hvp"][t])
        unread_is_zero(p, outs[t])
    assert D.same_bits(outs[D.DENSE], D.abi_hvp(p, s.g, s.u)), f"{case.id}: a repeated call gives other bits"
    nan = s.u.clone()
    nan[:, s.unused] = float("nan")
    assert D.same_bits(outs[D.DENSE], D.abi_hvp(p, s.g, nan)), f"{case.id}: the tangent of an atom nothing reads reaches h"
    if case.id in D.MISALIGNED:
        off = route(p, "hvp", aligned16=False)
        assert plan["vec4"] == 1 and off["vec4"] == 0
        assert D.same_bits(outs[D.DENSE], D.abi_hvp(p, s.g, s.u, misaligned=True)), f"{case.id}: the scalar stores give other bits"


def check_fwd(p, ref):
    case, s = p.case, p.s
    route(p, "fwd")
    feat = p.feat.cpu().numpy()                              # (written by abi_prepare's cvf_align_feature_fwd call, NaN before it)
    assert np.isfinite(feat).all(), f"{case.id}: features not fully written"
    for t, c in s.cols.items():
        held(case, "fwd", t, feat[:, c], ref.ref["fwd"][:, c], ref.bar["fwd"][t])
    pos = s.cols["position"]
    assert D.same_bits(feat[:, pos], s.traj[:, list(s.feats[0][1])].reshape(case.B, -1)), f"{case.id}: a position record is a copy"


def check_metric(p, ref):
    case, s = p.case, p.s
    plan = route(p, "metric")
    q, E = D.abi_metric(p, s.gk)
    q_ref, E_ref = ref.ref["metric"]
    assert q.shape == q_ref.shape and np.isfinite(q).all() and np.isfinite(E).all(), f"{case.id}: a valid output lane was not written"
    eq, eE = float(D.metric_q_errors(q, q_ref).max()), float((np.abs(E - E_ref) / E_ref).max())
    ERRORS.setdefault(case.id, {}).update({"metric/q": eq, "metric/q/bar": ref.bar["metric"]["q"], "metric/E": eE,
                                           "metric/E/bar": ref.bar["metric"]["E"]})
    print(f"[deriv] {case.id:20s} metric lg {plan['lg']} nets/pass {plan['rows_per_launch']} q {eq:.2e} (bar {ref.bar['metric']['q']:.2e}) "
          f"E {eE:.2e} (bar {ref.bar['metric']['E']:.2e})", flush=True)
    assert eq <= ref.bar["metric"]["q"] <= D.CEILING and eE <= ref.bar["metric"]["E"] <= D.CEILING, (case.id, eq, eE)
    q2, E2 = D.abi_metric(p, s.gk)
    assert D.same_bits(q, q2) and D.same_bits(E, E2), f"{case.id}: a repeated call gives other bits"


CHECKS = {"vjp": check_vjp, "rows": check_rows, "jvp": check_jvp, "hvp": check_hvp, "fwd": check_fwd, "metric": check_metric}
RUNS = [(c.id, run) for c in D.CASES for run in c.runs]


@pytest.mark.parametrize("cid,run", RUNS, ids=[f"{cid}-{run}" for cid, run in RUNS])
def test_instance_per_frame_and_type_vs_fp64(dev, cid, run):
    case = D.BY_ID[cid]
    CHECKS[run](prepared(case, dev), D.reference(case))
