"""The Python front end of the un-projection does with every call what it did before it was rebuilt from one family table: which op a call
reaches with which arguments, what it returns without a launch, what it refuses and how, what every family hands the C++ extension, the 72
schemas, their shape functions and the autograd formula -- all against tests/golden/frontend_calls.json, taken from the commit before the
rebuild by tests/frontend_record.py (its docstring says how to regenerate it).  No GPU: nothing launches."""
import json
import os

import pytest

import frontend_record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_calls.json")


@pytest.fixture(scope="module")
def clear():
    return json.loads(json.dumps(frontend_record.record()))               # (through JSON: tuples and lists compare equal)


@pytest.fixture(scope="module")
def recorded(clear):
    return frontend_record.flat(frontend_record.compact(clear))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return frontend_record.flat(json.load(fh))


def test_the_recorder_and_the_golden_hold_the_same_cases(recorded, golden, clear):
    assert sorted(recorded) == sorted(clear)                               # the golden's form drops no case
    assert sorted(set(recorded) - set(golden)) == [], "cases the golden lacks"
    assert sorted(set(golden) - set(recorded)) == [], "cases the recorder no longer produces"


def test_the_golden_holds_every_kind_of_case(golden):
    """the list of the golden's contents, so that a regenerated file cannot quietly lose a part"""
    fams, fns = frontend_record.FAMILIES, frontend_record.FUNCTIONS
    assert len(fams) == 18 and len(frontend_record.OPS) == 72
    for fn in fns:
        names = [k.split("/", 2)[2] for k in golden if k.startswith("door/%s/" % fn)]
        for want in ("plain", "mask", "weights", "weights+mask", "visible", "visible+mask", "conf", "conf+mask", "conf+visible", "conf+mask+visible",
                     "index", "lens auto", "lens gather", "var", "meanvar+mask", "meanvar+visible", "fp16 features", "out=bf16", "sum", "mean", "max",
                     "empty B=0", "empty zero extent", "empty M=0"):
            assert want in names, (fn, want)
        assert all("ops" in golden["door/%s/%s" % (fn, n)] and len(golden["door/%s/%s" % (fn, n)]["ops"]) == (0 if n.startswith("empty") else 1)
                   for n in names if not n.startswith("refuses")), fn
        refused = [n for n in names if n.startswith("refuses")]
        assert all("raises" in golden["door/%s/%s" % (fn, n)] for n in refused), fn
        assert len([n for n in refused if n.startswith("refuses 2:")]) >= 6
        said = " ".join(golden["door/%s/%s" % (fn, n)]["message"] for n in refused)
        for text in ("is not built yet (the next step of DESIGN.md 5.14)", "is not built yet (the next step of DESIGN.md 5.13)",
                     "is not built yet (the next step of DESIGN.md 5.12)", "is not supported yet (the next step of DESIGN.md 5.10)",
                     "has no weighted form (pass a view_mask, not view_weights)", "has no weighted form (pass a view_mask, not view_confidence)",
                     "view_weights together with view_confidence is not taken", "is outside [0, 2)", "at most 65535 per call",
                     "lens is not differentiable", "Unknown aggregation_method", "Unknown kernel variant", "has no CPU path"):
            assert text in said, (fn, text)
    gen = [k.split("/", 2)[2] for k in golden if k.startswith("door/VolumeGenerator/")]
    for want in ("view_mask", "view_weights", "view_confidence", "feature_index", "lens", "visible_only"):
        assert want in gen and "volume_pose" in golden["door/VolumeGenerator/" + want], want
    for fam in fams:
        for layout in ("planar auto", "channels-last C=4 gather", "channels-last C=6 gather"):
            for call in ("forward", "backward", "backward deterministic", "geometry defaults"):
                assert "native/%s/%s/%s" % (fam, layout, call) in golden, (fam, layout, call)
        assert "fake/" + fam in golden and "autograd/%s/all" % fam in golden and "autograd/%s/all deterministic" % fam in golden
    assert all("schema/" + op in golden for op in frontend_record.OPS)
    assert golden["schema/sha256"] == frontend_record.SCHEMA_SHA256       # of the 72 schema strings joined: as before the rebuild


def test_every_case_is_what_the_golden_says(recorded, golden, clear):
    differ = [k for k in sorted(set(recorded) & set(golden)) if recorded[k] != golden[k]]
    detail = "".join("\n%s\n  golden:   %s\n  recorded: %s" % (k, json.dumps(golden[k])[:600], json.dumps(clear[k])[:1500]) for k in differ[:5])
    assert not differ, "%d cases differ: %s%s" % (len(differ), differ[:40], detail)
