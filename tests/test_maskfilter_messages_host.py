"""No message of the four mask-filter kinds moved: the catalogue of tests/golden/make_maskfilter_messages_golden.py -- refused calls of the 16
public functions of the family with the library out of reach, and the four *_routes_emu programs on a fixed input -- replayed on the working
tree and compared, whole strings, with what tests/golden/maskfilter_messages.json recorded before the host path of the kinds was shared."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_maskfilter_messages_golden", os.path.join(ROOT, "tests", "golden", "make_maskfilter_messages_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

FUNCTIONS = ("maskfilter", "maskfilter_stems", "maskfilter_complex", "maskfilter_stereo",
             "maskfilter_batch", "maskfilter_stems_batch", "maskfilter_complex_batch", "maskfilter_stereo_batch",
             "maskfilter_ragged", "maskfilter_stems_ragged", "maskfilter_complex_ragged", "maskfilter_stereo_ragged",
             "pack_ragged_masks", "pack_ragged_stems_masks", "pack_ragged_complex_masks", "pack_ragged_stereo_masks")
EMUS = ("maskfilter_stems_routes_emu", "maskfilter_stems_ragged_routes_emu", "maskfilter_complex_routes_emu", "maskfilter_stereo_routes_emu")


@pytest.fixture(scope="module")
def golden():
    with open(maker.GOLDEN) as f:
        return json.load(f)


def test_the_golden_covers_the_family(golden):
    """The condition that keeps the comparison from passing on little: the 16 functions, each with refusals of its own, and the four programs."""
    assert set(golden["python"]) == set(FUNCTIONS) == set(maker.PYTHON_FUNCTIONS) and len(FUNCTIONS) == 16
    for fn, entries in golden["python"].items():
        refused = [e for e in entries if e["type"] == "ValueError"]
        assert len(entries) >= 3 and len(refused) >= 3, fn
        assert len({e["case"] for e in entries}) == len(entries), fn
        assert any(e["type"] in ("LibraryReached", "returned") for e in entries), fn   # (the checks let a good call through)
    assert set(golden["routes"]) == set(EMUS) == set(maker.ROUTES_EMUS)
    for name, rec in golden["routes"].items():
        assert rec["stdin"] == maker.routes_inputs()[name], name
        lines = rec["stdout"].strip().split("\n")
        assert sum(line == "taken" for line in lines) >= 2 and sum(line.startswith("refused") for line in lines) >= 6, name
    stereo = golden["routes"]["maskfilter_stereo_routes_emu"]["stdout"]
    assert "refused 2: " in stereo and "refused 1: " in stereo and "refused -1: " in stereo and "units " in stereo


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_python_messages(golden, fn):
    import zafx
    got = maker.record_python(maker.python_catalogue(zafx)[fn])
    want = golden["python"][fn]
    assert [e["case"] for e in got] == [e["case"] for e in want]
    for g, w in zip(got, want):
        assert g == w, (fn, g["case"])


@pytest.mark.parametrize("name", EMUS)
def test_routes_messages(golden, tmp_path_factory, name):
    exe = maker.build_emu(name, tmp_path_factory.mktemp(name))
    assert maker.run_emu(exe, golden["routes"][name]["stdin"]) == golden["routes"][name]["stdout"]
