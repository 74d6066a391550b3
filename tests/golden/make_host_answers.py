"""Records every answer the C ABI gives without a device, over a descriptor sweep that reaches every host route, into
host_answers_abi4.json (tests/test_host_answers_cpu.py recomputes the table from the current build and requires equality).

    python tests/golden/make_host_answers.py            # rewrite the table from the library that is built now

Only a change that is MEANT to move a byte count, a route or an error text re-records it; a refactor of the host code must not.

Per descriptor: the 13 workspace queries, selected_variant, forward_kernel_name, backward_supported, preferred_layout,
feature_layout_bytes for both destination layouts, and -- for every launching entry point whose workspace need is non-zero -- the
status and mvhmr_last_error() text of a call with dummy non-null pointers and a null workspace (it stops at the workspace check or
before it; nothing is launched).  A second section holds, for a few descriptors, one call per nulled pointer argument, the
"no gradient asked for" calls of the geometry entry points, and every entry point's answer to descriptors it refuses (bad
descriptors; quad layouts and the brick variant under a mask).

Layout of the file: "texts" interns the strings; "sweep" maps "shape,feat_dtype,out_dtype,layout,variant" to a list of
[methods, row] pairs, where `methods` names the aggregation methods ("0123" when the row does not depend on the method, which is
the usual case) and `row` is the flat list described by ROW; "calls" maps "descriptor|entry point|case" to [status, text].
"""
import collections
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from multiviewhmr_amd import _capi  # noqa: E402

OUT = os.path.join(HERE, "host_answers_abi%d.json" % _capi.ABI_VERSION)
DP, SZ = ctypes.c_void_p, ctypes.c_size_t

SHAPES = [  # B V C Hf Wf X Y Z
    (2, 4, 32, 24, 20, 8, 6, 5),            # under the 96-brick AUTO threshold
    (32, 4, 256, 96, 96, 64, 64, 64),       # the north star: k_fwd_ws, gated forward and backward
    (1, 4, 256, 96, 96, 64, 64, 64),        # batch 1 of it (channel split)
    (8, 4, 256, 12, 12, 16, 16, 16),        # the shipped 16^3 on 12 x 12 maps: AUTO takes the plane backward
    (32, 8, 256, 96, 96, 64, 64, 64),       # 8 views: view groups, 8 x 4 x 16 backward bricks
    (4, 3, 258, 96, 96, 64, 64, 64),        # 3 views (absent view slots), C = 258 (tail quad; channels-last refused)
    (4, 12, 32, 24, 24, 32, 32, 32),        # 12 views: gather only
    (3, 2, 6, 40, 30, 20, 24, 36),          # C = 6
    (32, 4, 32, 96, 96, 32, 32, 32),        # a 32^3 grid on 96 x 96 maps
    (2, 1, 8, 200, 200, 64, 64, 64),        # a single view
    (4, 5, 128, 300, 300, 64, 64, 32),      # maps too large for the plane kernel's LDS
]
METHODS = range(4)
STORAGE = ((_capi.F32, _capi.F32), (_capi.F16, _capi.F16), (_capi.F32, _capi.BF16), (_capi.F32, _capi.F16))   # the last one is refused
LAYOUTS = range(4)
VARIANTS = range(3)

_FWD = ["features", "proj"]
_BWD = ["grad_out", "features", "proj"]
_TENSOR, _CUBOID = ["coords"], ["rot", "center", "position", "sides"]
# entry point -> (the workspace query that sizes it, its pointer arguments between the descriptor and the workspace)
UNMASKED = collections.OrderedDict([
    ("forward", ("forward", _FWD + _TENSOR + ["out"])),
    ("forward_cuboid", ("forward", _FWD + _CUBOID + ["out"])),
    ("backward", ("backward", _BWD + _TENSOR + ["grad_features"])),
    ("backward_cuboid", ("backward", _BWD + _CUBOID + ["grad_features"])),
    ("backward_deterministic", ("backward_deterministic", _BWD + _TENSOR + ["grad_features"])),
    ("backward_cuboid_deterministic", ("backward_deterministic", _BWD + _CUBOID + ["grad_features"])),
    ("backward_geometry", ("backward_geometry", _BWD + _TENSOR + ["grad_proj", "grad_coords"])),
    ("backward_geometry_cuboid", ("backward_geometry_cuboid", _BWD + _CUBOID + ["grad_proj", "grad_rot", "grad_center"])),
])


def _with_mask(args):
    at = args.index("sides" if "sides" in args else "coords") + 1
    return args[:at] + ["view_mask"] + args[at:]


ENTRY = collections.OrderedDict(UNMASKED)
for _name, (_query, _args) in UNMASKED.items():
    ENTRY[_name + "_masked"] = (_name + "_masked", _with_mask(_args))
QUERIES = ["forward", "backward", "backward_geometry", "backward_deterministic", "backward_geometry_cuboid"] + [n + "_masked" for n in UNMASKED]
HOST = ["selected_variant", "forward_kernel_name", "backward_supported", "preferred_layout", "feature_layout_bytes(BVHWC)", "feature_layout_bytes(QUAD)"]
# a row: the QUERIES' answers, the HOST answers, then [status, text] of each ENTRY (in order) whose query answered non-zero
ROW = QUERIES + HOST + ["status, text of %s when its need is non-zero" % n for n in ENTRY]
assert len(QUERIES) == 13 and len(ENTRY) == 16

_POS, _SIDES = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)


def _lib():
    L = _capi.lib()
    for n in QUERIES:
        f = getattr(L, "mvhmr_unproject_%s_workspace_bytes" % n)
        f.argtypes, f.restype = [DP], SZ
    return L


def _desc(shape, agg, feat, out, layout, kernels, **kw):
    d = _capi.Desc()
    d.abi_version = _capi.ABI_VERSION
    (d.batch, d.views, d.channels, d.feat_h, d.feat_w, d.vol_x, d.vol_y, d.vol_z) = shape
    d.method, d.feat_dtype, d.out_dtype, d.feat_layout, d.variant = agg, feat, out, layout, kernels
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _query(L, d, name):
    return getattr(L, "mvhmr_unproject_%s_workspace_bytes" % name)(ctypes.byref(d))


def _call(L, d, name, null=()):
    """the entry point with dummy pointers the validation never dereferences (those named in `null`: null) and a null workspace"""
    ptrs = []
    for a in ENTRY[name][1]:
        if a in null:
            ptrs.append(None)
        else:
            ptrs.append(_POS if a == "position" else _SIDES if a == "sides" else DP(256))
    rc = getattr(L, "mvhmr_unproject_" + name)(ctypes.byref(d), *ptrs, None, SZ(0), None)
    return [rc, L.mvhmr_last_error().decode()]


def _row(L, d):
    a = ctypes.byref(d)
    need = collections.OrderedDict((n, _query(L, d, n)) for n in QUERIES)
    kernel = L.mvhmr_unproject_forward_kernel_name(a)
    row = list(need.values()) + [L.mvhmr_unproject_selected_variant(a), kernel.decode() if kernel else None, L.mvhmr_unproject_backward_supported(a),
                                 L.mvhmr_preferred_layout(a), L.mvhmr_feature_layout_bytes(a, _capi.LAYOUT_BVHWC),
                                 L.mvhmr_feature_layout_bytes(a, _capi.LAYOUT_QUAD)]
    for name, (query, _) in ENTRY.items():
        if need[query] > 0:
            row += _call(L, d, name)
    return row


# descriptors of the per-pointer section: each has a non-zero need at every entry point it is used for
CALL_DESCS = collections.OrderedDict([
    ("tiny planar", dict(shape=SHAPES[0], layout=_capi.LAYOUT_BVCHW)),
    ("north star planar", dict(shape=SHAPES[1], layout=_capi.LAYOUT_BVCHW)),
    ("north star quad", dict(shape=SHAPES[1], layout=_capi.LAYOUT_QUAD)),
    ("tiny channels-last f16", dict(shape=SHAPES[0], layout=_capi.LAYOUT_BVHWC, feat_dtype=_capi.F16, out_dtype=_capi.F16)),
])
REFUSED = collections.OrderedDict([
    ("abi_version 3", dict(abi_version=3)), ("batch 0", dict(batch=0)), ("method 7", dict(method=7)), ("17 views", dict(views=17)),
    ("feat bf16", dict(feat_dtype=_capi.BF16)), ("layout 4", dict(feat_layout=4)), ("variant 3", dict(variant=3)),
    ("quad", dict(feat_layout=_capi.LAYOUT_QUAD)), ("quad log2e", dict(feat_layout=_capi.LAYOUT_QUAD_LOG2E)),
    ("brick", dict(variant=_capi.VARIANT["brick"])), ("quad brick", dict(feat_layout=_capi.LAYOUT_QUAD, variant=_capi.VARIANT["brick"])),
])


def _calls(L):
    out = collections.OrderedDict()
    for label, kw in CALL_DESCS.items():
        d = _desc(kw["shape"], 0, kw.get("feat_dtype", _capi.F32), kw.get("out_dtype", _capi.F32), kw["layout"], _capi.VARIANT["auto"])
        for name, (query, args) in ENTRY.items():
            masked = name.endswith("_masked")
            if masked and kw["layout"] == _capi.LAYOUT_QUAD:
                continue                            # refused before the pointers are looked at everywhere: see REFUSED
            if _query(L, d, query) == 0:
                continue
            for a in args:
                out["%s|%s|null %s" % (label, name, a)] = _call(L, d, name, null=(a,))
            if "geometry" in name:
                grads = [a for a in args if a.startswith("grad_") and a != "grad_out"]
                out["%s|%s|no gradient asked for" % (label, name)] = _call(L, d, name, null=grads)
                out["%s|%s|no gradient asked for, null features" % (label, name)] = _call(L, d, name, null=grads + ["features"])
            out["%s|%s|null features and %s" % (label, name, args[3])] = _call(L, d, name, null=("features", args[3]))
    # descriptors an entry point refuses whatever its workspace: the null workspace is never reached, or is what stops the call
    for label, kw in REFUSED.items():
        for shape in (SHAPES[0], SHAPES[1]):
            d = _desc(shape, 0, _capi.F32, _capi.F32, _capi.LAYOUT_BVCHW, _capi.VARIANT["auto"], **kw)
            for name, (query, _) in ENTRY.items():
                need = _query(L, d, query)
                stops_early = label not in ("quad", "quad log2e", "brick", "quad brick") or name.endswith("_masked")
                if stops_early or need > 0:
                    out["%s %s|%s|refused" % (label, "x".join(map(str, shape)), name)] = _call(L, d, name) + [need]
    return out


def compute():
    """the table as it is stored (texts interned), and the coverage of the sweep"""
    L = _lib()
    texts, index = [], {}

    def intern(x):
        if not isinstance(x, str):
            return x
        if x not in index:
            index[x] = len(texts)
            texts.append(x)
        return "#%d" % index[x]

    sweep = collections.OrderedDict()
    nonzero = collections.Counter()
    host = collections.Counter()
    for shape, (fd, od), layout, variant in itertools.product(SHAPES, STORAGE, LAYOUTS, VARIANTS):
        groups = []                                 # [methods, row], methods with the same row together
        for method in METHODS:
            row = [intern(x) for x in _row(L, _desc(shape, method, fd, od, layout, variant))]
            for i, n in enumerate(QUERIES):
                nonzero[n] += row[i] > 0
            host[tuple(row[13:17])] += 1
            for g in groups:
                if g[1] == row:
                    g[0] += str(method)
                    break
            else:
                groups.append([str(method), row])
        sweep[",".join(map(str, shape + (fd, od, layout, variant)))] = groups
    calls = collections.OrderedDict((k, [intern(x) for x in v]) for k, v in _calls(L).items())
    table = collections.OrderedDict([("abi_version", _capi.ABI_VERSION), ("row", ROW), ("texts", texts), ("sweep", sweep), ("calls", calls)])
    return table, nonzero, host


def check_coverage(table, nonzero, host):
    """the sweep must not prove nothing: every query answers non-zero somewhere, every forward kernel is chosen somewhere"""
    never = [n for n in QUERIES if nonzero[n] == 0]
    kernels = {table["texts"][int(k[1][1:])] for k in host if k[1] is not None}
    missing = {"k_fwd_ws", "k_fwd_brick", "k_fwd_brick_groups", "k_fwd_gather"} - kernels
    if never or missing:
        raise SystemExit("the sweep is too narrow: queries that are zero everywhere %s, forward kernels never chosen %s" % (never, sorted(missing)))


def dumps(table):
    """one line per descriptor / call, so that a re-recording diffs row by row"""
    lines = ['{"abi_version": %d,' % table["abi_version"], '"row": %s,' % json.dumps(table["row"]), '"texts": [']
    lines += [",\n".join("  " + json.dumps(t) for t in table["texts"]), '],']
    for section in ("sweep", "calls"):
        lines.append('"%s": {' % section)
        lines.append(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table[section].items()))
        lines.append("}," if section == "sweep" else "}}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    table, nonzero, host = compute()
    n = sum(len(m) for g in table["sweep"].values() for m, _ in g)
    print("%d descriptors in %d rows, %d calls, %d texts" % (n, sum(len(g) for g in table["sweep"].values()), len(table["calls"]), len(table["texts"])))
    for q in QUERIES:
        print("  %-45s non-zero for %4d descriptors, %3d distinct values" % (q, nonzero[q], len({r[QUERIES.index(q)] for g in table["sweep"].values() for _, r in g})))
    print("  %d distinct (selected_variant, forward_kernel_name, backward_supported, preferred_layout)" % len(host))
    check_coverage(table, nonzero, host)
    with open(OUT, "w") as f:
        f.write(dumps(table))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
