"""The `ndt_hip` driver over every output sink and every way of combining them, against the record of the driver before its host
layer was rebuilt around one frame request (tests/golden/driver_matrix.json, written by tests/golden/make_golden_driver.py on an
MI355X): every file a run leaves under images/, depth/ and beside them (--raw) byte for byte (sha256 and size), and every line on
stdout in order, with only the clock's seconds and the count of visible devices masked.  16x9, frames 0..1 of a two-document YAML
scene: nine rows do not divide among 2 or 3 contexts, two frames cover the per-frame names and the animated PNG's canvas.  For
`-j 2` the files alone are compared (the workers' lines interleave).  Needs a real MI355X: run with `pytest -m gpu`.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_driver", os.path.join(HERE, "golden", "make_golden_driver.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def record():
    with open(recorder.RECORD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every case run once, each under its own time limit; a run that fails or hangs ends the matrix there."""
    assert os.path.exists(recorder.DRIVER), "ndt_amd/host/ndt_hip is not built"
    return recorder.run_matrix(recorder.DRIVER, str(tmp_path_factory.mktemp("matrix")))


def test_the_record_holds_the_cases_of_the_recorder(record):
    assert record["base"] == recorder.BASE and tuple(record["documents"]) == recorder.DOCUMENTS
    assert {n: c["flags"] for n, c in record["cases"].items()} == dict(recorder.CASES)
    for name, c in record["cases"].items():
        assert c["files"], name


@pytest.mark.parametrize("name", [name for name, _ in recorder.CASES])
def test_driver_writes_and_says_what_it_did_before(record, runs, name):
    want_files, want_lines = recorder.compared(name, record["cases"][name])
    got_files, got_lines = recorder.compared(name, runs[name])
    assert sorted(got_files) == sorted(want_files)
    for path in want_files:
        assert got_files[path] == want_files[path], path
    assert got_lines == want_lines
