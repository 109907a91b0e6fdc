"""The dispatch record: tools/dispatch_record.py walks a fixed list of mips_search calls across every threshold the host
dispatch branches on (storage, pitch, k, query count, output form, the knobs, the fast_skip countdown, the pool of 16 on a
large index at pitch 1024); tests/dispatch_record.json holds, per call, the kernel instance that answered it and what the
margin check counted.  A change of the dispatch has to edit that file on purpose
(python tools/dispatch_record.py --write tests/dispatch_record.json)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("dispatch_record", os.path.join(ROOT, "tools", "dispatch_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _expected():
    with open(os.path.join(ROOT, "tests", "dispatch_record.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("which", ["small", "large"])
def test_dispatch_record(which):
    tool = _tool()
    calls = tool.small_calls() if which == "small" else tool.large_calls()
    labels = [tool.label(c) for c in calls]
    exp = [e for e in _expected() if e["call"] in set(labels)]
    assert [e["call"] for e in exp] == labels          # the committed record lists exactly these calls, in this order
    got = tool.record((which,))
    diff = [(g["call"], g["kernel"], g["stats"], e["kernel"], e["stats"]) for g, e in zip(got, exp)
            if g["kernel"] != e["kernel"] or g["stats"] != e["stats"]]
    assert not diff, diff
