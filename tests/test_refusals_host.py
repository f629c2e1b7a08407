"""The refusals of the C ABI, pinned: tests/golden/refusals.json holds the return code and the full rt_last_error(NULL) text of a table
of refused calls (tests/golden/make_refusals.py: every options header too short, unset or with an unknown flag bit, the first value-range
refusal of every host-only check function, every device entry point with ctx null), recorded once. The built library must answer each
of them with the same code and the same text, byte for byte. No device is needed."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _table():
    spec = importlib.util.spec_from_file_location("make_refusals", os.path.join(GOLDEN, "make_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_match_the_pinned_table(pkg):
    table = _table()
    with open(table.FIXTURE) as f:
        pinned = json.load(f)
    got = table.record(pkg)
    assert [r["case"] for r in got] == [r["case"] for r in pinned], "the table and its fixture list different cases: record it again"
    assert len(pinned) >= 80 and all(r["code"] != pkg._abi.RT_OK and r["error"] for r in pinned)
    for g, p in zip(got, pinned):
        assert (g["code"], g["error"]) == (p["code"], p["error"]), p["case"]
