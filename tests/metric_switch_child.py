"""Child process of tests/test_metric_cases_gpu.py: the instances of ``metric_rows_kernel`` behind the process-wide developer
switches, which the library reads once per process - ``python -m tests.metric_switch_child waves16`` under
``CVF_METRIC_WAVES=16`` (the three 16-wave instances) or ``... pre5`` under ``CVF_METRIC_PRE=5`` (``<16, 8, 5, true>``).
Runs the cases of ``metric_cases.SWITCH_CASES`` that need the switch (tests/metric_cases.py: run_and_check) and ends with the
first failure's status."""
import os
import sys


def main(which):
    want = {"waves16": ("CVF_METRIC_WAVES", "16"), "pre5": ("CVF_METRIC_PRE", "5")}[which]
    assert os.environ.get(want[0]) == want[1], f"{which}: start me with {want[0]}={want[1]}"
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    import torch
    from tests import metric_cases as M
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    cases = [c for c in M.SWITCH_CASES if (c.waves == 16) == (which == "waves16")]
    assert cases
    seen = set()
    for c in cases:
        plan, _, _ = M.run_and_check(c, dev)
        seen.add((plan["F"], plan["waves"], plan["geo_pre"], plan["multi"]))
    assert seen == ({(16, 16, 2, 1), (8, 16, 2, 1), (4, 16, 2, 1)} if which == "waves16" else {(16, 8, 5, 1)}), seen
    print(f"[metric] child {which}: {len(cases)} cases ok", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
