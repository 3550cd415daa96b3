"""The Python evaluator against its characterisation snapshot (tools/make_eval_snapshot.py): on one fixed scene, in all five modes,
`Omni3Deval` evaluate / accumulate / summarize, `_derive_results`, `bootstrap`, a proximity pass, the four `*_groups` pair passes with
their warnings and the short form of `Omni3DEvaluator` must give what tests/golden/eval_snapshot_<target>.json recorded: the numbers and
printed text verbatim, every table by shape, dtype and sha256 of its bytes, and per phase the names handed to `HipLibrary.call` in
order.  The two files were recorded before the evaluator module was split (`emu` on the host emulator, `gfx950` on the MI355X, where
two recordings were identical byte for byte: every table is reproducible, none is compared rounded).  `Omni3DEvaluationHelper` is not
covered here; its own tests in test_{bev,dist,let,bootstrap}_eval.py and test_datasets_io.py are."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_eval_snapshot", os.path.join(ROOT, "tools", "make_eval_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _differences(want, got, where=""):
    """paths at which two JSON trees differ"""
    if isinstance(want, dict) and isinstance(got, dict):
        out = [where + "/" + k for k in want.keys() ^ got.keys()]
        for k in want.keys() & got.keys():
            out += _differences(want[k], got[k], where + "/" + k)
        return out if list(want) == list(got) or out else [where + " (key order)"]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [p for i, (w, g) in enumerate(zip(want, got)) for p in _differences(w, g, "%s[%d]" % (where, i))]
    return [] if want == got and type(want) is type(got) else ["%s: %r != %r" % (where, want, got)]


SECTIONS = ("2D", "3D", "BEV", "DIST", "LET", "groups", "short_form")


def _run(lib, target, section):
    tool = _tool()
    assert tool.SECTIONS == SECTIONS
    with open(tool.snapshot_path(target)) as f:
        want = json.load(f)
    assert tuple(want) == SECTIONS
    got = tool.record_section(lib, section)
    diff = _differences(want[section], got)
    assert not diff, "\n".join(diff[:40])
    assert got == want[section]


@pytest.mark.parametrize("section", SECTIONS)
def test_eval_snapshot_emulated(emu_lib, section):
    _run(emu_lib, "emu", section)


@pytest.mark.gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_eval_snapshot_gpu(hip_lib, section):
    _run(hip_lib, "gfx950", section)
