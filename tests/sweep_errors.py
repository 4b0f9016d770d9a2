"""The optional error report of the GPU sweeps (tests/test_ef_sweep_gpu.py, tests/test_ae_sweep_gpu.py): with CVF_SWEEP_ERRORS
set to a path, every sweep module of one pytest run adds its {case id: {quantity: error}} table to one JSON file there.  The
first module to write in a run replaces whatever an earlier run left, so no entry outlives its case."""
import json
import os

_written = set()   # paths this process has already started


def write(errors):
    path = os.environ.get("CVF_SWEEP_ERRORS")
    if not path:
        return
    table = {}
    if path in _written and os.path.exists(path):
        with open(path) as f:
            table = json.load(f)
    _written.add(path)
    table.update(errors)
    with open(path, "w") as f:
        json.dump(table, f, indent=1)
