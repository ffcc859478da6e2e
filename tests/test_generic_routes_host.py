"""CPU test of the route predicates of the generic decoder geometries -- TwoDimPlanesModel.generic_route, generic_train_route,
generic_arithmetic, generic_frame_route and train_utils._generic_occupancy -- over the product of everything they read: the three handles
(unset, 0, 1), dec_channels, model.arithmetic, gradients, a frozen decoder, planes that require gradients, jitter, the deterministic mode, a
built grid.  tests/generic_route_table.json was written by tools/generic_route_table.py on the commit before the predicates were folded
onto shared helpers; this tree must answer every row of it.  No GPU is touched."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("generic_route_table", os.path.join(ROOT, "tools", "generic_route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_row_of_the_recorded_table(pkg, tool, monkeypatch):
    monkeypatch.delenv("NVSR_DETERMINISTIC", raising=False)
    with open(os.path.join(ROOT, "tests", "generic_route_table.json")) as fh:
        want = json.load(fh)
    got = tool.table(pkg)
    assert json.loads(json.dumps(got["axes"])) == want["axes"], "the axes of the tool and of the recorded table differ"
    assert len(got["rows"]) == len(want["rows"]) == 3 ** 3 * 5 * 2 ** 7
    wrong = [i for i, (a, b) in enumerate(zip(got["rows"], want["rows"])) if a != b]
    assert not wrong, "%d rows differ; the first: %s: this tree %s, recorded %s" % (
        len(wrong), tool.describe(wrong[0]), got["rows"][wrong[0]], want["rows"][wrong[0]])
    assert torch.cuda.is_available() or not torch.cuda.is_initialized()


def test_the_table_sees_every_answer():
    """the recording is not vacuous: each predicate gives both of its answers somewhere in the product"""
    with open(os.path.join(ROOT, "tests", "generic_route_table.json")) as fh:
        rows = json.load(fh)["rows"]
    for column, letters in enumerate(("FL", "FL", "hs", "TO", "GN")):
        assert {r[column] for r in rows} == set(letters), (column, letters)
