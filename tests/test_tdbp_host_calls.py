"""The back-projection wrappers' host layer, pinned call by call (sarx/_tdbp_host.py and the five sarx/tdbp*.py wrappers): no device.

tests/_tdbp_host_recorder.py drives every wrapper against a stub context and renders each library call, alloc, upload, download
and release in order.  tests/golden/tdbp_host_calls.json is that record as the wrappers made it when each of them still did its
host work itself; the shared host layer must make the same calls with the same values in the same order."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_host_recorder as rec  # noqa: E402

PKG = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "sarx")
WRAPPERS = ("tdbp", "tdbp_search", "tdbp_pair", "tdbp_pair_search", "tdbp_multi")


@pytest.fixture(scope="module")
def recorded():
    return rec.golden()


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "tdbp_host_calls.json")) as f:
        return json.load(f)


def test_the_record_covers_every_form_of_every_wrapper(recorded):
    ok = recorded["ok"]
    for prefix, at_least in (("gpu", 4), ("search", 5), ("pair ", 12), ("multi", 20), ("pair_search", 5), ("resolve", 4)):
        assert sum(name.startswith(prefix) for name in ok) >= at_least, prefix
    assert all(name in recorded["launch fails"] for name, case in ok.items() if "raises" not in case)


def test_every_wrapper_makes_the_pinned_calls(recorded, pinned):
    """Exact: names, scalars, parameter-block bytes, the fp64 values behind geometry and hypothesis pointers, which buffer every
    other pointer is, allocs, uploads, downloads and releases in order, and what the caller sees of the result (route, lags,
    v_ambiguity, shapes, dtypes, owner flags, the NaN / -1 fill of a report outside the grid)."""
    assert recorded["fp64"] == pinned["fp64"]
    assert sorted(recorded["ok"]) == sorted(pinned["ok"])
    for name, case in recorded["ok"].items():
        assert case == pinned["ok"][name], name


def test_a_failing_launch_raises_and_leaves_the_pinned_trace(recorded, pinned):
    """Every launching case again with its launch entry returning -1.  One case of the golden file was recorded from the shared
    host layer, not from the wrappers before it: ``tdbp_pair(device_output=True)`` used to keep its device buffer when the launch
    raised (its ``finally`` covered the downloaded form only), and now releases it as ``tdbp_multi`` always did - one more
    "release" line and a count of 1 in place of 0.  Every other case is the earlier wrappers' trace."""
    assert sorted(recorded["launch fails"]) == sorted(pinned["launch fails"])
    for name, case in recorded["launch fails"].items():
        assert case.get("raises") == "SarxError", name
        assert case == pinned["launch fails"][name], name
    assert "release dev2" in recorded["launch fails"]["pair dev device_output"]["trace"]


@pytest.mark.parametrize("section", ["ok", "launch fails"])
def test_every_buffer_a_wrapper_allocates_is_released_exactly_once(recorded, section):
    """By the time the result's release() has run and the plan is closed: nothing leaks, nothing is released twice, and no buffer of
    the caller's (device raw, a device slot, d_image, a device stack) is released at all."""
    for name, case in recorded[section].items():
        assert all(n == 1 for n in case["released"].values()), (name, case["released"])
        assert case["caller's released"] == 0, name


def test_refusals_keep_their_exception_type(recorded):
    ok = recorded["ok"]
    refused = {name for name, case in ok.items() if case.get("raises") == "ValueError"}
    for name in ("gpu host d_image", "pair mixed", "pair device_output host", "pair device_output complex128", "pair transposed",
                 "pair mis-shaped", "multi not whole pulses", "multi raws and offsets differ", "multi mixed", "pair_search bad source",
                 "resolve slot without capacity"):
        assert name in refused, name
    assert ok["pair_search overflowed slot"]["raises"] == ok["resolve overflowed slot"]["raises"] == "SarxError"
    assert not [(n, t[0]) for n in refused for t in ok[n]["trace"] if isinstance(t, list) and t[0] in rec.LAUNCHES]      # refused before any launch


def test_no_wrapper_imports_a_private_name_of_another_wrapper():
    import re
    for mod in WRAPPERS:
        text = open(os.path.join(PKG, mod + ".py")).read()
        for other, names in re.findall(r"^from \.(tdbp\w*) import (.+)$", text, flags=re.M):
            private = [n.strip() for n in names.split(",") if n.strip().startswith("_")]
            assert not private, (mod, other, private)
