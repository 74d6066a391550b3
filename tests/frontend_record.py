"""What the Python front end of the un-projection (multiviewhmr_amd/aggregation.py) does with a call, written down without a GPU:

    door/...      which mvhmr:: op `unprojection` / `unprojection_cuboid` / `VolumeGenerator.forward` reach, with which arguments -- or what they
                  return without a launch, or the exception they raise (type and message)
    native/...    which op of the C++ extension every family's forward / backward / backward_geometry calls, its arguments by name with the
                  schema's defaults filled in (so positional and keyword calls compare equal), and what comes back
    schema/...    the schema string of all 72 registered ops
    fake/...      their output shapes and dtypes under FakeTensorMode
    autograd/...  which backward ops the registered formula runs, with which want_* flags, and which inputs get a gradient of which shape

`record()` returns {case name: JSON-able value}; `compact()` replaces the long argument lists by digests, case by case, so that the golden
stays small.  tests/test_frontend_cpu.py compares that with tests/golden/frontend_calls.json, which
`python tests/frontend_record.py tests/golden/frontend_calls.json` writes.  Only public names, torch.ops.mvhmr.*, aggregation._native and the
pinned attributes of aggregation._OPS[...] are used, so the file runs unchanged on an older aggregation.py: the golden was taken from the
commit before the front end was rebuilt from one family table, by running this file in a `git worktree` of it.

A tensor is written as "dtype[shape]@device" (+ "!" when not contiguous, + "=values" for a non-floating tensor of at most 16 elements, so mask
bytes and indices are held)."""
import contextlib
import hashlib
import inspect
import json
import os
import sys
import unittest.mock as mock

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multiviewhmr_amd import _capi, aggregation  # noqa: E402

B, V, C, H, W, S, M = 2, 3, 4, 8, 8, 4, 3
INDEX = [1, 0, 1]
FUNCTIONS = ("unprojection", "unprojection_cuboid")
FAMILIES = tuple(f + k for f in FUNCTIONS for k in ("", "_masked")) + tuple(                 # (the order they were first registered in:
    f + k for k in ("_weighted", "_visible", "_confidence", "_confidence_visible", "_shared", "_lens", "_moments") for f in FUNCTIONS)   # the digest's)
OPS = tuple(f + s for f in FAMILIES for s in ("", "_backward", "_backward_deterministic", "_backward_geometry"))
SCHEMA_SHA256 = "ce63d5b122c1b75eff8f35a6b8a3e4f5c434b7224c6fde8347741df23f14ec8f"           # of the 72 schema strings joined by newlines


def enc(x):
    if torch.is_tensor(x):
        s = "%s%s@%s" % (str(x.dtype).replace("torch.", ""), list(x.shape), x.device.type)
        if not x.is_contiguous():
            s += "!"
        if not (x.dtype.is_floating_point or x.dtype.is_complex) and x.numel() <= 16 and x.device.type == "cpu" and type(x) is torch.Tensor:
            s += "=" + json.dumps(x.to(torch.int64).flatten().tolist(), separators=(",", ":"))
        return s
    if isinstance(x, (list, tuple)):
        return [enc(v) for v in x]
    if isinstance(x, dict):
        return {k: enc(v) for k, v in x.items()}
    if isinstance(x, (torch.dtype, torch.device)):
        return str(x)
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return repr(x)


# ------------------------------------------------------------------------------------------------ front door
class _Intercept(TorchDispatchMode):
    """every mvhmr:: op is written down and answered with a one-element tensor; nothing launches"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.namespace != "mvhmr":
            return func(*args, **(kwargs or {}))
        self.calls.append({"op": func.name(), "args": enc(list(args)), "kwargs": enc(dict(kwargs or {}))})
        return torch.zeros(args[0].shape[0], 3) if "triangulate_dlt" in func.name() else torch.zeros(1)


def _outcome(call, on_device=True):
    """-> what `call()` reached: the intercepted ops and the result, or the exception.  on_device: CPU tensors say they are on a HIP device"""
    patch = mock.patch.object(torch.Tensor, "is_cuda", property(lambda s: True)) if on_device else contextlib.nullcontext()
    with patch, _Intercept() as seen:
        try:
            out = call()
        except Exception as e:  # noqa: BLE001 -- the type and the message are the record
            return {"raises": type(e).__name__, "message": str(e), "ops": seen.calls}
    return {"returns": enc(out), "ops": seen.calls}


def _base(fn, n=B, volumes=None, dtype=torch.float32, vol=(S, S, S)):
    """the positional arguments of `fn` for n samples (volumes: with a feature_index)"""
    m = n if volumes is None else volumes
    lead = (torch.zeros(n, V, C, H, W, dtype=dtype), torch.zeros(n, V, 3, 4))
    if fn == "unprojection":
        return lead + (torch.zeros((m,) + tuple(vol) + (3,)),)
    return lead + (torch.zeros(m, 3, 3), torch.zeros(m, 3), (-1.0, -1.0, -1.0), np.array([2.0, 2.0, 2.0]), tuple(vol))


def _mask(dtype=torch.bool):
    return torch.tensor([[1, 0, 1], [1, 1, 1]]).to(dtype)


def _options():
    """name -> (aggregation_method, keyword arguments, volumes); fresh tensors per call"""
    w, conf = torch.ones(B, V), torch.ones(B, V, H, W)
    idx, lens = torch.tensor(INDEX), torch.zeros(B, V, 10)
    return {
        "plain": ("softmax", {}, None),
        "sum": ("sum", {}, None), "mean": ("mean", {}, None), "max": ("max", {}, None),
        "max+mask": ("max", dict(view_mask=_mask()), None),
        "variant=gather": ("softmax", dict(variant="gather"), None),
        "variant=brick": ("softmax", dict(variant="brick"), None),
        "out=bf16": ("softmax", dict(out_dtype=torch.bfloat16), None),
        "out=f16": ("softmax", dict(out_dtype=torch.float16), None),
        "mask": ("softmax", dict(view_mask=_mask()), None),
        "mask int64": ("mean", dict(view_mask=_mask(torch.int64) * 7), None),
        "weights": ("softmax", dict(view_weights=w), None),
        "weights f64": ("sum", dict(view_weights=w.double()), None),
        "weights+mask": ("mean", dict(view_weights=w, view_mask=_mask()), None),
        "visible": ("softmax", dict(visible_only=True), None),
        "visible truthy": ("softmax", dict(visible_only=1), None),
        "visible+mask": ("max", dict(visible_only=True, view_mask=_mask()), None),
        "conf": ("softmax", dict(view_confidence=conf), None),
        "conf f16": ("sum", dict(view_confidence=conf.half()), None),
        "conf+mask": ("mean", dict(view_confidence=conf, view_mask=_mask()), None),
        "conf+visible": ("softmax", dict(view_confidence=conf, visible_only=True), None),
        "conf+mask+visible": ("sum", dict(view_confidence=conf, view_mask=_mask(), visible_only=True), None),
        "index": ("softmax", dict(feature_index=idx), M),
        "index int32 gather": ("mean", dict(feature_index=idx.to(torch.int32), variant="gather"), M),
        "lens auto": ("softmax", dict(lens=lens, variant="auto"), None),
        "lens gather": ("sum", dict(lens=lens, variant="gather"), None),
        "lens brick f64": ("max", dict(lens=lens.double(), variant="brick"), None),
        "var": ("var", {}, None),
        "var gather bf16": ("var", dict(variant="gather", out_dtype=torch.bfloat16), None),
        "meanvar": ("meanvar", {}, None),
        "meanvar+mask": ("meanvar", dict(view_mask=_mask()), None),
        "meanvar+visible": ("meanvar", dict(visible_only=True), None),
        "var+mask+visible": ("var", dict(view_mask=_mask(torch.uint8), visible_only=True), None),
    }


def _door_calls(out):
    for fn in FUNCTIONS:
        f = getattr(aggregation, fn)
        for name, (method, kw, volumes) in _options().items():
            out["door/%s/%s" % (fn, name)] = _outcome(lambda: f(*_base(fn, volumes=volumes), method, **kw))
        out["door/%s/fp16 features" % fn] = _outcome(lambda: f(*_base(fn, dtype=torch.float16), "softmax"))
        out["door/%s/fp16 features+mask" % fn] = _outcome(lambda: f(*_base(fn, dtype=torch.float16), "softmax", view_mask=_mask()))
        out["door/%s/f64 geometry" % fn] = _outcome(lambda: f(*[t.double() if torch.is_tensor(t) and i else t for i, t in enumerate(_base(fn))]))
        out["door/%s/geometry requires grad" % fn] = _outcome(
            lambda: f(*[t.requires_grad_(True) if torch.is_tensor(t) else t for t in _base(fn)], "sum", view_weights=torch.ones(B, V, requires_grad=True)))
        # launch-free returns
        empty = {"B=0": dict(n=0), "zero extent": dict(vol=(S, 0, S)), "B=0 meanvar": dict(n=0), "zero extent meanvar bf16": dict(vol=(0, S, S))}
        for name, how in empty.items():
            method = "meanvar" if "meanvar" in name else "softmax"
            kw = dict(out_dtype=torch.bfloat16) if "bf16" in name else {}
            out["door/%s/empty %s" % (fn, name)] = _outcome(lambda: f(*_base(fn, **how), method, **kw))
        out["door/%s/empty M=0" % fn] = _outcome(lambda: f(*_base(fn, volumes=0), feature_index=torch.zeros(0, dtype=torch.int64)))
        out["door/%s/empty index zero extent" % fn] = _outcome(lambda: f(*_base(fn, volumes=M, vol=(S, S, 0)), "sum", feature_index=torch.tensor(INDEX)))
        out["door/%s/empty index B=0 f16" % fn] = _outcome(
            lambda: f(*_base(fn, n=0, volumes=0, dtype=torch.float16), feature_index=torch.zeros(0, dtype=torch.int32)))
        out["door/%s/empty B=0 mask" % fn] = _outcome(lambda: f(*_base(fn, n=0), view_mask=torch.zeros(0, V, dtype=torch.bool)))


def _refusals():
    """name -> (aggregation_method, keyword arguments, volumes, runs behind the is_cuda patch)"""
    w, conf = torch.ones(B, V), torch.ones(B, V, H, W)
    idx, lens, mask = torch.tensor(INDEX), torch.zeros(B, V, 10), _mask()
    r = {}
    for method in ("var", "meanvar"):
        for name, kw in (("weights", dict(view_weights=w)), ("conf", dict(view_confidence=conf)), ("index", dict(feature_index=idx)), ("lens", dict(lens=lens))):
            r["%s+%s" % (method, name)] = (method, kw, M if name == "index" else None, True)
    r["max+weights"] = ("max", dict(view_weights=w), None, True)
    r["max+conf"] = ("max", dict(view_confidence=conf), None, True)
    r["weights+conf"] = ("sum", dict(view_weights=w, view_confidence=conf), None, True)
    r["visible+weights"] = ("sum", dict(visible_only=True, view_weights=w), None, True)
    for name, kw in (("mask", dict(view_mask=mask)), ("weights", dict(view_weights=w)), ("visible", dict(visible_only=True)), ("conf", dict(view_confidence=conf)),
                     ("index", dict(feature_index=idx))):
        r["lens+" + name] = ("softmax", dict(lens=lens, **kw), M if name == "index" else None, True)
    for name, kw in (("mask", dict(view_mask=mask)), ("weights", dict(view_weights=w)), ("visible", dict(visible_only=True)), ("conf", dict(view_confidence=conf))):
        r["index+" + name] = ("softmax", dict(feature_index=idx, **kw), M, True)
    r["mask a list"] = ("softmax", dict(view_mask=[[1, 0, 1], [1, 1, 1]]), None, True)
    r["mask float"] = ("softmax", dict(view_mask=w), None, True)
    r["mask shape"] = ("softmax", dict(view_mask=torch.ones(B, V + 1, dtype=torch.bool)), None, True)
    r["weights a list"] = ("softmax", dict(view_weights=[[1.0] * V] * B), None, True)
    r["weights int"] = ("softmax", dict(view_weights=torch.ones(B, V, dtype=torch.int32)), None, True)
    r["weights shape"] = ("softmax", dict(view_weights=torch.ones(V, B)), None, True)
    r["conf an array"] = ("softmax", dict(view_confidence=np.ones((B, V, H, W), np.float32)), None, True)
    r["conf int"] = ("softmax", dict(view_confidence=torch.ones(B, V, H, W, dtype=torch.uint8)), None, True)
    r["conf shape"] = ("softmax", dict(view_confidence=torch.ones(B, V, W + 1, H)), None, True)
    r["index a list"] = ("softmax", dict(feature_index=INDEX), M, True)
    r["index float"] = ("softmax", dict(feature_index=idx.float()), M, True)
    r["index bool"] = ("softmax", dict(feature_index=idx.bool()), M, True)
    r["index 2-D"] = ("softmax", dict(feature_index=idx[None]), M, True)
    r["index M>65535"] = ("softmax", dict(feature_index=torch.zeros(65536, dtype=torch.int32)), M, True)
    r["index past B (cpu)"] = ("softmax", dict(feature_index=torch.tensor([1, 2, 0])), M, False)
    r["index negative (cpu)"] = ("softmax", dict(feature_index=torch.tensor([1, -1, 5])), M, False)
    r["index volumes mismatch"] = ("softmax", dict(feature_index=torch.tensor([1, 0])), M, True)
    r["lens a list"] = ("softmax", dict(lens=[0.0] * 10), None, True)
    r["lens int"] = ("softmax", dict(lens=lens.to(torch.int64)), None, True)
    r["lens shape"] = ("softmax", dict(lens=torch.zeros(B, V, 9)), None, True)
    r["lens requires grad"] = ("softmax", dict(lens=torch.zeros(B, V, 10, requires_grad=True)), None, True)
    r["unknown method"] = ("median", {}, None, True)
    r["unknown variant"] = ("softmax", dict(variant="fast"), None, True)
    r["out=f64"] = ("softmax", dict(out_dtype=torch.float64), None, True)
    r["no HIP device"] = ("softmax", {}, None, False)
    r["no HIP device, mask"] = ("softmax", dict(view_mask=mask), None, False)
    # two mistakes at once: who wins
    r["2: var+weights+lens"] = ("var", dict(view_weights=w, lens=lens), None, True)
    r["2: meanvar+lens shape"] = ("meanvar", dict(lens=torch.zeros(B, V, 9)), None, True)
    r["2: lens shape+index float"] = ("softmax", dict(lens=torch.zeros(B, V, 9), feature_index=idx.float()), M, True)
    r["2: lens+mask float"] = ("softmax", dict(lens=lens, view_mask=w), None, True)
    r["2: lens+index 2-D"] = ("softmax", dict(lens=lens, feature_index=idx[None]), M, True)
    r["2: index+mask shape"] = ("softmax", dict(feature_index=idx, view_mask=torch.ones(V, B, dtype=torch.bool)), M, True)
    r["2: index M>65535+weights"] = ("softmax", dict(feature_index=torch.zeros(65536, dtype=torch.int32), view_weights=w), M, True)
    r["2: mask shape+weights int"] = ("softmax", dict(view_mask=torch.ones(V, B, dtype=torch.bool), view_weights=torch.ones(B, V, dtype=torch.int32)), None, True)
    r["2: max+weights+visible"] = ("max", dict(view_weights=w, visible_only=True), None, True)
    r["2: visible+weights+conf int"] = ("sum", dict(visible_only=True, view_weights=w, view_confidence=torch.ones(B, V, H, W, dtype=torch.uint8)), None, True)
    r["2: max+weights+conf"] = ("max", dict(view_weights=w, view_confidence=conf), None, True)
    r["2: weights shape+conf+weights"] = ("sum", dict(view_weights=torch.ones(V, B), view_confidence=conf), None, True)
    r["2: mask shape+unknown method"] = ("median", dict(view_mask=torch.ones(V, B, dtype=torch.bool)), None, True)
    r["2: conf shape+unknown variant"] = ("sum", dict(view_confidence=torch.ones(B, V, 1, 1), variant="fast"), None, True)
    r["2: index past B+no HIP device"] = ("softmax", dict(feature_index=torch.tensor([0, 0, 9])), M, False)
    r["2: mask float+no HIP device"] = ("softmax", dict(view_mask=w), None, False)
    return r


def _door_refusals(out):
    for fn in FUNCTIONS:
        f = getattr(aggregation, fn)
        for name, (method, kw, volumes, on_device) in _refusals().items():
            out["door/%s/refuses %s" % (fn, name)] = _outcome(lambda: f(*_base(fn, volumes=volumes), method, **kw), on_device)

        def bent(change, method="softmax", **kw):
            args = list(_base(fn))
            change(args)
            return _outcome(lambda: f(*args, method, **kw))

        def put(i, v):
            return lambda args: args.__setitem__(i, v)

        out["door/%s/refuses features an array" % fn] = bent(put(0, np.zeros((B, V, C, H, W), np.float32)))
        out["door/%s/refuses proj an array" % fn] = bent(put(1, np.zeros((B, V, 3, 4), np.float32)))
        out["door/%s/refuses placing an array" % fn] = bent(put(2, np.zeros((B, 3, 3), np.float32)))
        out["door/%s/refuses features 4-D" % fn] = bent(put(0, torch.zeros(B, C, H, W)))
        out["door/%s/refuses proj shape" % fn] = bent(put(1, torch.zeros(B, V, 4, 4)))
        out["door/%s/refuses placing shape" % fn] = bent(put(2, torch.zeros(B + 1, 3, 3) if fn == "unprojection_cuboid" else torch.zeros(B, S, S, S, 2)))
        out["door/%s/refuses proj on another device" % fn] = bent(put(1, torch.zeros(B, V, 3, 4, device="meta")))
        out["door/%s/refuses 2: features an array+mask float" % fn] = bent(put(0, np.zeros((B, V, C, H, W), np.float32)), view_mask=torch.ones(B, V))
        out["door/%s/refuses 2: features an array+visible+weights" % fn] = bent(put(0, np.zeros((B, V, C, H, W), np.float32)), visible_only=True,
                                                                               view_weights=torch.ones(B, V))
        out["door/%s/refuses 2: features an array+var+lens" % fn] = bent(put(0, np.zeros((B, V, C, H, W), np.float32)), "var", lens=torch.zeros(B, V, 10))
        out["door/%s/refuses 2: features 4-D+mask shape" % fn] = bent(put(0, torch.zeros(B, C, H, W)), view_mask=torch.ones(V, B, dtype=torch.bool))
        out["door/%s/refuses 2: proj shape+weights int" % fn] = bent(put(1, torch.zeros(B, V, 4, 4)), view_weights=torch.ones(B, V, dtype=torch.int32))
        out["door/%s/refuses 2: placing shape+unknown variant" % fn] = bent(put(2, torch.zeros(B + 1, 3, 3, 3)), variant="fast")


# ------------------------------------------------------------------------------------------------ VolumeGenerator.forward
def _generator(**kw):
    torch.manual_seed(0)
    gen = aggregation.VolumeGenerator(volume_size=S, input_channels=C, output_channels=C, device="cpu", **kw)
    gen.fused_conv = False
    gen.eval()
    pose = []
    real, sig = gen.volume_pose, inspect.signature(gen.volume_pose)

    def volume_pose(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        pose.append({k: enc(v) for k, v in bound.arguments.items() if k not in ("batch", "proj_matricies_org") and v is not None})
        return real(*args, **kwargs)

    gen.volume_pose = volume_pose
    return gen, pose


def _batch(volumes=None, **kw):
    n = B if volumes is None else volumes
    return dict(images=torch.empty((B, V, 32, 32, 3), device="meta"), keypoints_3d=torch.zeros(n, 17, 3),
                cameras_packed=dict(K=torch.eye(3).repeat(B, V, 1, 1).double(), Rt=torch.eye(3, 4).repeat(B, V, 1, 1).double()), **kw)


def _generator_calls(out):
    w, conf = torch.ones(B, V), torch.ones(B, V, H, W)
    idx, lens, mask = torch.tensor(INDEX), torch.zeros(B, V, 10), _mask()
    cases = {
        "plain": ({}, {}, None),
        "view_mask": ({}, dict(view_mask=mask), None),
        "view_weights": ({}, dict(view_weights=w), None),
        "view_weights+view_mask": ({}, dict(view_weights=w, view_mask=mask), None),
        "view_confidence": ({}, dict(view_confidence=conf), None),
        "view_confidence+view_mask": ({}, dict(view_confidence=conf, view_mask=mask), None),
        "feature_index": ({}, dict(feature_index=idx), M),
        "lens": (dict(lens_distortion=True), dict(lens=lens), None),
        "lens off, batch has one": ({}, dict(lens=lens), None),
        "visible_only": (dict(visible_only=True), {}, None),
        "visible_only+view_mask": (dict(visible_only=True), dict(view_mask=mask), None),
        "visible_only+view_confidence": (dict(visible_only=True), dict(view_confidence=conf), None),
        "meanvar+view_mask bf16": (dict(aggregation_method="meanvar", volume_dtype=torch.bfloat16), dict(view_mask=mask), None),
        "var+visible_only": (dict(aggregation_method="var", visible_only=True), {}, None),
        "triangulated view_weights+view_mask": (dict(use_triangulation=True), dict(view_weights=w, view_mask=mask), None),
        "triangulated feature_index": (dict(use_triangulation=True), dict(feature_index=idx), M),
        # one thing wrong
        "refuses var+view_weights": (dict(aggregation_method="var"), dict(view_weights=w), None),
        "refuses meanvar+lens": (dict(aggregation_method="meanvar", lens_distortion=True), dict(lens=lens), None),
        "refuses max+view_weights": (dict(aggregation_method="max"), dict(view_weights=w), None),
        "refuses max+view_confidence": (dict(aggregation_method="max"), dict(view_confidence=conf), None),
        "refuses view_weights+view_confidence": ({}, dict(view_weights=w, view_confidence=conf), None),
        "refuses visible_only+view_weights": (dict(visible_only=True), dict(view_weights=w), None),
        "refuses feature_index+view_mask": ({}, dict(feature_index=idx, view_mask=mask), M),
        "refuses feature_index+visible_only": (dict(visible_only=True), dict(feature_index=idx), M),
        "refuses feature_index past B (cpu)": ({}, dict(feature_index=torch.tensor([1, 0, 2])), M),
        "refuses lens+view_mask": (dict(lens_distortion=True), dict(lens=lens, view_mask=mask), None),
        "refuses lens+feature_index": (dict(lens_distortion=True), dict(lens=lens, feature_index=idx), M),
        "refuses lens shape": (dict(lens_distortion=True), dict(lens=torch.zeros(B, V, 9)), None),
        "refuses view_mask float": ({}, dict(view_mask=w), None),
        "refuses view_mask shape": ({}, dict(view_mask=torch.ones(V, B, dtype=torch.bool)), None),
        "refuses view_weights int": ({}, dict(view_weights=torch.ones(B, V, dtype=torch.int64)), None),
        "refuses view_confidence shape": ({}, dict(view_confidence=torch.ones(B, V, H + 1, W)), None),
    }
    for name, (how, extra, volumes) in cases.items():
        gen, pose = _generator(**how)
        res = _outcome(lambda: gen(torch.zeros(B, V, C, H, W), torch.zeros(B, V, 3, 4), _batch(volumes, **extra)), on_device="(cpu)" not in name)
        if "raises" not in res:                               # (a failing call may check before or after the pose: not pinned)
            res["volume_pose"] = pose
        out["door/VolumeGenerator/" + name] = res


# ------------------------------------------------------------------------------------------------ ops -> extension
def _bind(schema, args, kwargs):
    """the call's arguments by the schema's names, defaults filled in"""
    params = list(schema.arguments)
    bound = {p.name: p.default_value for p in params if p.has_default_value()}
    assert len(args) <= len([p for p in params if not p.kwarg_only]), (schema.name, len(args))
    for p, a in zip(params, args):
        bound[p.name] = a
    for k, v in kwargs.items():
        assert k in {p.name for p in params} and k not in {p.name for p in params[:len(args)]}, (schema.name, k)
        bound[k] = v
    assert set(bound) == {p.name for p in params}, (schema.name, sorted({p.name for p in params} - set(bound)))
    return {p.name: bound[p.name] for p in params}


class _Spy:
    """stands in for torch.ops.mvhmr_native: writes every call down and answers with tensors of the shapes the extension returns"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        schema = getattr(self.real, name).default._schema

        def op(*args, **kwargs):
            bound = _bind(schema, args, kwargs)
            if name.endswith("_backward_geometry"):
                diff = [k[len("want_"):] for k in bound if k.startswith("want_")]
                res = tuple(torch.zeros(tuple(bound[k].shape) if bound["want_" + k] else (0,)) for k in diff)
            else:
                res = torch.zeros(1)
            # the leading arguments (through `variant`: the same long list in every call of a case) as a digest, to keep the golden small
            names = list(bound)
            cut = names.index("variant") + 1
            lead = json.dumps(enc({k: bound[k] for k in names[:cut]}), sort_keys=True)
            self.calls.append({"op": name, "lead": hashlib.sha256(lead.encode()).hexdigest()[:16], "args": enc({k: bound[k] for k in names[cut:]})})
            return res
        return op


def _channels_last(t):
    return t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


def _family_args(name, features, variant, absent_mask=False, moments=2):
    """the positional arguments of mvhmr::<name>, from its registered schema"""
    n = M if name.endswith("_shared") else B
    values = dict(features=features, proj=torch.zeros(B, V, 3, 4), coords=torch.zeros(n, S, S, S, 3), rot=torch.zeros(n, 3, 3), center=torch.zeros(n, 3),
                  view_mask=None if absent_mask else _mask(torch.uint8), view_weights=torch.ones(B, V), view_confidence=torch.ones(B, V, H, W),
                  feature_index=torch.tensor(INDEX, dtype=torch.int32), lens=torch.zeros(B, V, 10), position=[-1.0, -1.0, -1.0], sides=[2.0, 2.0, 2.0],
                  vol=[S, S + 1, S + 2], visible_only=True, moments=moments, method=_capi.AGG["mean"], out_dtype=_capi.F32, variant=variant)
    return [values[a.name] for a in getattr(torch.ops.mvhmr, name).default._schema.arguments]


def _native_calls(out):
    spy = _Spy(aggregation._native())
    layouts = {"planar auto": (lambda: torch.zeros(B, V, C, H, W), _capi.VARIANT["auto"]),
               "planar gather": (lambda: torch.zeros(B, V, C, H, W), _capi.VARIANT["gather"]),
               "channels-last C=4 gather": (lambda: _channels_last(torch.zeros(B, V, 4, H, W)), _capi.VARIANT["gather"]),
               "channels-last C=6 gather": (lambda: _channels_last(torch.zeros(B, V, 6, H, W)), _capi.VARIANT["gather"]),
               "fp16 planar auto": (lambda: torch.zeros(B, V, C, H, W, dtype=torch.float16), _capi.VARIANT["auto"])}

    def run(key, call):
        del spy.calls[:]
        try:
            res = call()
            out[key] = {"calls": list(spy.calls), "returns": enc(res)}
        except Exception as e:  # noqa: BLE001
            out[key] = {"calls": list(spy.calls), "raises": type(e).__name__, "message": str(e)}

    with mock.patch.object(aggregation, "_native", lambda: spy):
        for name in FAMILIES:
            fam = aggregation._OPS[name]
            optional_mask = "?" in str(getattr(torch.ops.mvhmr, name).default._schema.arguments[fam.tensors.index("view_mask")].type) if fam.masked else False
            for lname, (make, variant) in layouts.items():
                grad_out = torch.zeros(1).expand(2, 3)                      # not contiguous: the ops hand the extension a contiguous one
                variants = [("", dict())] + ([(" no mask", dict(absent_mask=True))] if optional_mask else []) + (
                    [(" var", dict(moments=1))] if name.endswith("_moments") else [])
                for vname, how in variants:
                    key = "native/%s/%s%s/" % (name, lname, vname)
                    args = _family_args(name, make(), variant, **how)
                    run(key + "forward", lambda: fam.forward(*args))
                    run(key + "backward", lambda: fam.backward(False, grad_out, *args))
                    run(key + "backward deterministic", lambda: fam.backward(True, grad_out, *args))
                    n = len(fam.grads)
                    run(key + "geometry defaults", lambda: fam.backward_geometry(grad_out, *args))
                    for want in [(True,) * n] + [tuple(i == j for j in range(n)) for i in range(n)]:
                        which = "+".join(g for g, w in zip(fam.grads, want) if w)
                        run(key + "geometry " + which, lambda: fam.backward_geometry(grad_out, *args, *want))
        f, p, c = torch.zeros(B, V, C, H, W), torch.zeros(B, V, 3, 4), torch.zeros(B, S, S, S, 3)
        run("native/_op_backward", lambda: aggregation._op_backward(torch.zeros(1), f, p, c, 0, _capi.F32, 0))


# ------------------------------------------------------------------------------------------------ registration
def _schemas(out):
    strings = [str(getattr(torch.ops.mvhmr, op).default._schema) for op in OPS]
    for op, s in zip(OPS, strings):
        out["schema/" + op] = s
    out["schema/sha256"] = hashlib.sha256("\n".join(strings).encode()).hexdigest()


def _fake_shapes(out):
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in FAMILIES:
        fam = aggregation._OPS[name]
        with FakeTensorMode():
            for tag, how, dt in (("", {}, _capi.F32), (" bf16", {}, _capi.BF16), (" var", dict(moments=1), _capi.F16)):
                args = _family_args(name, torch.zeros(B, V, C, H, W), 0, **how)
                args[-2] = dt
                fwd = getattr(torch.ops.mvhmr, name)(*args)
                go = torch.zeros(fwd.shape)
                res = {"forward": enc(fwd), "backward": enc(getattr(torch.ops.mvhmr, name + "_backward")(go, *args)),
                       "backward_deterministic": enc(getattr(torch.ops.mvhmr, name + "_backward_deterministic")(go, *args))}
                n = len(fam.grads)
                geo = getattr(torch.ops.mvhmr, name + "_backward_geometry")
                res["geometry defaults"] = enc(geo(go, *args))
                for want in [(True,) * n] + [tuple(i == j for j in range(n)) for i in range(n)]:
                    res["geometry " + "+".join(g for g, w in zip(fam.grads, want) if w)] = enc(geo(go, *args, *want))
                out["fake/%s%s" % (name, tag)] = res


class _Watch(TorchDispatchMode):
    """lets every op run, remembers the mvhmr:: ones with their bool arguments (the want_* flags)"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.namespace == "mvhmr":
            schema = func._schema
            flags = {a.name: v for a, v in zip(schema.arguments, args) if a.name.startswith("want_")}
            flags.update({k: v for k, v in (kwargs or {}).items() if k.startswith("want_")})
            self.calls.append({"op": func.name(), "n_args": len(args), "want": flags})
        return func(*args, **(kwargs or {}))


def _autograd(out):
    for name in FAMILIES:
        fam = aggregation._OPS[name]
        diff = ("features",) + tuple(fam.grads)
        floats = [t for t in fam.tensors if t not in ("view_mask", "feature_index")]
        runs = [(d, (d,), False) for d in diff] + [("all", diff, False), ("all deterministic", diff, True),
                                                   ("every float tensor", tuple(floats), False)]
        for tag, which, deterministic in runs:
            with torch.device("meta"):
                args = _family_args(name, torch.zeros(B, V, C, H, W), 0)
            names = [a.name for a in getattr(torch.ops.mvhmr, name).default._schema.arguments]
            for i, n in enumerate(names):
                if n in which:
                    args[i].requires_grad_(True)
            was = torch.are_deterministic_algorithms_enabled()
            torch.use_deterministic_algorithms(deterministic)
            case = {}
            try:
                with _Watch() as seen:
                    res = getattr(torch.ops.mvhmr, name)(*args)
                    res.sum().backward()
            except Exception as e:  # noqa: BLE001 -- a broken formula is a differing case, not a crash of the recorder
                case = {"raises": type(e).__name__, "message": str(e)}
            finally:
                torch.use_deterministic_algorithms(was)
            grads = {n: enc(a.grad) for n, a in zip(names, args) if torch.is_tensor(a) and a.grad is not None}
            out["autograd/%s/%s" % (name, tag)] = dict(case, ops=seen.calls, grads=grads)


def record():
    out = {}
    _door_calls(out)
    _door_refusals(out)
    _generator_calls(out)
    _native_calls(out)
    _schemas(out)
    _fake_shapes(out)
    _autograd(out)
    return out


def digest(value):
    return hashlib.sha256(json.dumps(value, sort_keys=True).encode()).hexdigest()[:12]


def compact(cases):
    """The golden's form of record(), which keeps every case and stays small: a door/ case in the clear but for a digest of each reached op's
    arguments; every other case as a digest (the joined schema digest in full), nested by the parts of its name below section/family"""
    out = {}
    for key, value in cases.items():
        if key.startswith("door/"):
            out[key] = dict(value, ops=[{"op": c["op"], "args": digest([c["args"], c["kwargs"]])} for c in value["ops"]])
            continue
        section, family, *rest = key.split("/")
        parts, node = [section + "/" + family] + rest, out
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = value if key == "schema/sha256" else digest(value)
    return out


def flat(compacted, prefix=""):
    """compact()'s result with one entry per case again: {case name: value or digest}"""
    out = {}
    for key, value in compacted.items():
        if isinstance(value, dict) and not key.startswith("door/"):
            out.update(flat(value, prefix + key + "/"))
        else:
            out[prefix + key] = value
    return out


if __name__ == "__main__":
    lines = [json.dumps(k) + ":" + json.dumps(v, sort_keys=True, separators=(",", ":")) for k, v in sorted(compact(record()).items())]
    with open(sys.argv[1], "w") as fh:
        fh.write("{\n" + ",\n".join(lines) + "\n}\n")
