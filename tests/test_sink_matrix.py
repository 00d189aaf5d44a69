"""Every delivering entry of the C ABI -- the plain frame, OpenEXR, supersampled, animated PNG, denoised and AO-shaded, each into
every sink it has -- against the record of the library before its delivery half was folded into one set of tails
(tests/golden/sink_matrix_parent.json, written by tests/golden/make_golden_sinks.py on an MI355X): sha256 and length of every
array and file returned for a 24 x 10 frame and its cyclic shard, the ray counts, the stages' launch counters, and for every
refusal (a NULL output, a buffer one byte short, a shard without rows, K = 0 and 9, a misaligned device pointer, a size beyond the
file format's bound) the return code, the message byte for byte, and that the output was left alone.  Nothing of the record is
masked unless the record names it.  Needs a real MI355X: run with `pytest -m gpu`.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_sinks", os.path.join(HERE, "golden", "make_golden_sinks.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def record():
    with open(recorder.RECORD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(record):
    """Every case run once, one context a stage"""
    return recorder.masked(recorder.run_matrix(), record["masked"])


def test_the_record_holds_the_cases_of_the_recorder(record):
    assert record["entries"] == [e.name for e in recorder.ENTRIES] and sorted(record["cases"]) == sorted(record["entries"])
    assert (record["scene"], record["frame"], record["shard"]) == (recorder.SCENE, [recorder.W, recorder.H], recorder.SHARD)
    for name, c in record["cases"].items():
        assert "returned" in c and "refusals" in c, name
        for kind, r in c["refusals"].items():
            assert r["untouched"], (name, kind)
            assert r["rc"] != 0 or kind == "zero_rows", (name, kind)


@pytest.mark.parametrize("name", [e.name for e in recorder.ENTRIES])
def test_entry_delivers_and_refuses_what_it_did_before(record, cases, name):
    want, got = record["cases"][name], cases[name]
    different = recorder.differing(want, got)
    for path in different:
        print("%s%s differs" % (name, path))
    assert not different
