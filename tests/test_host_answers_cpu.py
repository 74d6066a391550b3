"""Every answer the C ABI gives without a device -- the 13 workspace queries, the route questions and the status + mvhmr_last_error()
text of calls that stop at or before the workspace check -- recomputed over the recorded descriptor sweep and compared, entry for
entry, with tests/golden/host_answers_abi4.json.  No other test pins the exact byte counts and error texts across routes; this is
what lets a change to the host route (csrc/capi.hip's plan functions) be reviewed.  tests/golden/make_host_answers.py records it."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def answers():
    spec = importlib.util.spec_from_file_location("make_host_answers", os.path.join(GOLDEN, "make_host_answers.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.OUT) as f:
        recorded = json.load(f)
    table, nonzero, host = rec.compute()
    rec.check_coverage(table, nonzero, host)
    return rec, recorded, json.loads(rec.dumps(table))


def _resolve(x, texts):
    return texts[int(x[1:])] if isinstance(x, str) and x.startswith("#") else x


def test_the_sweep_is_the_recorded_one(answers):
    rec, recorded, now = answers
    assert recorded["abi_version"] == now["abi_version"] and recorded["row"] == now["row"]
    assert list(recorded["sweep"]) == list(now["sweep"]) and list(recorded["calls"]) == list(now["calls"])
    n = len(rec.SHAPES) * len(rec.STORAGE) * len(rec.LAYOUTS) * len(rec.VARIANTS)
    assert len(now["sweep"]) == n and n * len(rec.METHODS) >= 2112


def test_every_descriptor_gets_the_recorded_answers(answers):
    rec, recorded, now = answers
    wrong = []
    for key, groups in recorded["sweep"].items():
        want = {m: [_resolve(x, recorded["texts"]) for x in row] for methods, row in groups for m in methods}
        got = {m: [_resolve(x, now["texts"]) for x in row] for methods, row in now["sweep"][key] for m in methods}
        assert sorted(want) == sorted(got) == [str(m) for m in rec.METHODS], key
        for m in want:
            if want[m] != got[m]:
                at = next((i for i, (a, b) in enumerate(zip(want[m], got[m])) if a != b), min(len(want[m]), len(got[m])))
                wrong.append("%s method %s, entry %d (%s): recorded %r, now %r" % (
                    key, m, at, rec.ROW[at] if at < 19 else "entry-point calls", want[m][at:at + 2], got[m][at:at + 2]))
    assert not wrong, "%d descriptors answer differently:\n%s" % (len(wrong), "\n".join(wrong[:20]))


def test_every_refused_call_gets_the_recorded_status_and_text(answers):
    rec, recorded, now = answers
    wrong = []
    for key, want in recorded["calls"].items():
        want = [_resolve(x, recorded["texts"]) for x in want]
        got = [_resolve(x, now["texts"]) for x in now["calls"][key]]
        if want != got:
            wrong.append("%s: recorded %r, now %r" % (key, want, got))
        assert want[0] != 0, key                    # none of these calls may get as far as a launch
    assert not wrong, "%d calls answer differently:\n%s" % (len(wrong), "\n".join(wrong[:20]))


def test_the_extension_registers_six_unprojection_ops():
    """mvhmr_native:: holds the six unmasked names (view_mask and deterministic are trailing, defaulted arguments), the two DLT ops and
    abi_version -- no per-mask or per-mode copies"""
    import torch
    from multiviewhmr_amd import build
    torch.ops.load_library(build.build_ext())
    ops = {s.name.split("::")[1] for s in torch._C._jit_get_all_schemas() if s.name.startswith("mvhmr_native::")}
    unproject = {"unprojection" + c + k for c in ("", "_cuboid") for k in ("", "_backward", "_backward_geometry")}
    assert ops == unproject | {"triangulate_dlt", "triangulate_dlt_backward", "abi_version"}
    for name in unproject:
        args = {a.name: a for a in getattr(torch.ops.mvhmr_native, name).default._schema.arguments}
        assert str(args["view_mask"].type) == "Optional[Tensor]" and args["view_mask"].default_value is None and args["view_mask"].has_default_value()
        assert ("deterministic" in args) == name.endswith("_backward")
        if name.endswith("_backward"):
            assert args["deterministic"].default_value is False
