"""CPU (-m "not gpu"): the references of tests/test_shared_ef_task_gpu.py (tests/shared_ef_task_cases.py) are fit to decide ``cvec`` -
the fp64 eigenvalues of every step case and of every step of the training loops are pairwise apart by far more than the bars."""
import numpy as np

from tests import shared_ef_task_cases as S


def _gap(eig):
    eig = np.asarray(eig, dtype=np.float64)
    return float(np.diff(np.sort(eig)).min() / np.abs(eig).max())


def test_step_cases_have_separated_eigenvalues():
    import __graft_entry__  # noqa: F401
    ref, bars = S.step_reference()
    assert all(0 < b < 1e-2 for b in bars.values()), bars
    for case, (lv, eig, cvec, grad) in ref.items():
        print(f"[shared-task] {S.case_id(case)}: smallest eigenvalue gap {_gap(eig):.2e} (eig bar {bars['eig']:.2e})")
        assert _gap(eig) > 20 * bars["eig"], (case, eig)
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0


def test_training_loops_have_separated_eigenvalues():
    import __graft_entry__  # noqa: F401
    ref, bars = S.train_reference()
    for case, want in ref.items():
        k = case[2]
        assert want["rows"].shape == (S.TRAIN["num_epochs"], 3, 3 + k)       # two train steps and one test step per epoch
        gap = min(_gap(row[3:]) for ep in want["rows"] for row in ep)
        print(f"[shared-task] train {S.case_id(case)}: smallest eigenvalue gap {gap:.2e}, bars {bars[case]}")
        assert all(0 < b < 1e-1 for b in bars[case].values()), bars[case]
        assert gap > 20 * bars[case]["rows"], (case, gap)
