"""The premise of the exact lattice rig (tests/lattice_rig.py), checked on the CPU for every rig the GPU file uses:

  * oracle agreement: oracle/unproject_np.py (float32), the rig's float64 oracle and the C oracle give the same bits, forward and
    backward; the float32 backward is also accumulated tap by tap in two different random orders -- if fp32 arithmetic in ANY order has
    the float64 answer's bits, a kernel's order of additions and of float atomics cannot matter;
  * budget: sum |terms| / quantum < 2^24 for every compared element, from the oracle's tap table;
  * coverage, so that no rig is trivially easy (each from the tap table):
      - at least 50 % of voxel-views have a live tap;
      - at least 30 % of live taps are fractional (weight strictly between 0 and 1);
      - taps exist with ix exactly 0, exactly W - 1, in (-1, 0) and in (W - 1, W), and the same for iy.  A condition no volume axis of
        the rig can reach (lattice_rig.edge_feasible: half a lattice step is a whole pixel or more on a map much finer than the
        volume -- only the two in-between bands can be out of reach) is not required of that rig;
      - with V > 2 at least one view lies behind the camera;
      - for `max`, at most 15 % of the compared elements are tied."""
import numpy as np
import pytest

import lattice_rig as rig
from oracle import cport, unproject_np

METHODS = ("sum", "max", "mean")


def _methods(name):
    V = rig.RIGS[name]["V"]
    return [m for m in METHODS if m != "mean" or V in (1, 2, 4, 8)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, ref64):
    """got (float32) has exactly the bits of the float64 reference cast once (-0.0 and +0.0 are told apart too)"""
    got = np.asarray(got)
    assert got.dtype == np.float32
    return np.array_equal(_bits(got), _bits(np.asarray(ref64).astype(np.float32)))


def _shuffled_backward32(feats, proj, coords, grad, method, seed):
    """the float32 backward with every (voxel, tap) contribution added one by one, in a random order"""
    B, V, C, H, W = feats.shape
    s, tables = unproject_np.per_view_samples(feats, proj, coords)
    g = grad.reshape(B, 1, C, -1).astype(np.float32)
    if method == "sum":
        ds = np.broadcast_to(g, s.shape)
    elif method == "mean":
        ds = np.broadcast_to(g / np.float32(V), s.shape)
    else:
        ds = g * (np.arange(V)[None, :, None, None] == s.argmax(1)[:, None])
    gf = np.zeros((B, V, C, H * W), np.float32)
    rng = np.random.default_rng(seed)
    for (b, v), (off, w, ok) in tables.items():
        order = rng.permutation(off.size)
        flat_off = off.ravel()[order]
        for c in range(C):
            contrib = (ds[b, v, c][None] * w).astype(np.float32).ravel()[order]
            np.add.at(gf[b, v, c], flat_off, contrib)              # unbuffered: one fp32 addition per tap, in this order
    return gf.reshape(feats.shape)


@pytest.mark.parametrize("name", sorted(rig.RIGS))
def test_the_three_oracles_agree_bit_for_bit(name):
    feats, proj, coords, _ = rig.problem(name)
    for method in _methods(name):
        out64, grad, gf64, res = rig.reference(name, method)
        assert out64.dtype == np.float64 and gf64.dtype == np.float64
        assert _same_bits(unproject_np.forward(feats, proj, coords, method), out64), (name, method, "numpy fp32 forward")
        assert _same_bits(cport.forward(feats, proj, coords, method), out64), (name, method, "C forward")
        assert _same_bits(cport.backward(grad, feats, proj, coords, method), gf64), (name, method, "C backward")
        assert _same_bits(unproject_np.backward(grad, feats, proj, coords, method), gf64), (name, method, "numpy fp32 backward")
        for seed in (1, 2):
            assert _same_bits(_shuffled_backward32(feats, proj, coords, grad, method, seed), gf64), (name, method, "shuffled", seed)


@pytest.mark.parametrize("name", sorted(rig.RIGS))
def test_budget_and_coverage(name):
    cfg = rig.RIGS[name]
    H, W, V, vol = cfg["H"], cfg["W"], cfg["V"], cfg["vol"]
    for method in _methods(name):
        res = rig.reference(name, method)[3]
        rig.assert_budget(res, "%s %s" % (name, method))
        assert 0 < res["fwd_budget"] < rig.LIMIT and 0 < res["bwd_budget"] < rig.LIMIT
    res = rig.reference(name, "max")[3]
    st = res["stats"]
    assert st["live"] >= 0.5 * st["voxel_views"], (name, st)
    assert st["frac_taps"] >= 0.3 * st["live_taps"], (name, st)
    for row, span, keys in ((0, W, ("ix_hi", "ix_lo", "ixW", "ix0")), (1, H, ("iy_hi", "iy_lo", "iyH", "iy0"))):
        for role, key in zip(rig.EDGE_ROLES, keys):
            reachable = any(rig.edge_feasible(role, extent, span) for extent in vol)
            if reachable:
                assert st[key] > 0, (name, key, st)
            else:                                                    # no d = 1 lattice point of any axis lies in that band: not required
                assert role in ("hi", "lo"), (name, key, st)
    if V > 2:
        assert st["behind"] > 0, (name, st)
    assert res["tied"].mean() <= 0.15, (name, float(res["tied"].mean()))


def test_option_rigs_keep_their_budget():
    """the option routes' rigs as tests/test_lattice_gpu.py builds them (lattice_rig.option_cases): budget of the forward, the feature
    backward and -- on the small rig -- of grad_weights / grad_confidence"""
    for tag, name, method, kw in rig.option_cases():
        res = rig.option_reference(tag)
        rig.assert_budget(res, tag)


# ----------------------------------------------------------------------------------------------- the geometry path
"""The premise of the geometry rigs (lattice_rig.GEO_RIGS: maps with power-of-two H and W, so that kx = (W - 1) / H and ky = (H - 1) / W
are dyadic), for `sum`, `max` and power-of-two `mean`:

  * the rig's float64 geometry oracle, tests/geomgrad_oracle.py (written independently, from the forward's fp32 positions) and an fp32
    numpy restatement of k_bwd_geom's order that rounds after EVERY operation agree bit for bit; the restatement's sum over voxels runs
    in two different random orders;
  * geo_budget < 2^24;
  * no rig is trivially easy: >= 60 % of the compared grad_coords and of grad_proj are non-zero, <= 15 % `max` ties; over the set of
    rigs, live voxel-views lie in each border band, exactly on pixel 0 and on the last pixel, behind the camera and at z == 0;
  * the rigs SEE the slips the GPU tests are there to catch: the restatement with one of them applied no longer has the oracle's bits."""
import geomgrad_oracle                                            # noqa: E402

F32 = np.float32
GEO_PLAIN = [n for n in sorted(rig.GEO_RIGS) if "M" not in rig.GEO_RIGS[n] and n != "geo_conf"]


def _geo_methods(name):
    V = rig.GEO_RIGS[name]["V"]
    return [m for m in METHODS if m != "mean" or V & (V - 1) == 0]


def _fma(a, b, c):
    """fmaf: the product is exact in float64 (24 + 24 bits), one rounding to fp32 at the end"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _kernel_order32(feats, proj, coords, grad, method, seed, slip=None):
    """k_bwd_geom (csrc/unproject_geom_bwd.hip) and make_geo_rec (csrc/geom_bwd_common.h) in numpy fp32, one rounding per operation, in
    the kernel's order; the channel sum runs channel by channel and the voxel sum of grad_proj in the random order of `seed`, both in
    fp32 (the kernel keeps a fixed tree and float64 across blocks: any order must do on the rig).
    slip: None, or one deliberate mistake -- 'x1_lt' (xin1 = x1 < W - 1), 'no_value_mask' (a clamped tap keeps its value), 'swap_k'
    (kx and ky exchanged).  -> grad_proj (B,V,3,4), grad_coords (B,X,Y,Z,3) fp32"""
    B, V, C, H, W = feats.shape
    vol = coords.shape[1:4]
    N = int(np.prod(vol))
    rng = np.random.default_rng(seed)
    gp = np.zeros((B, V, 3, 4), F32)
    gc = np.zeros((B, N, 3), F32)
    kx, ky = F32(W - 1) / F32(H), F32(H - 1) / F32(W)
    if slip == "swap_k":
        kx, ky = ky, kx
    for b in range(B):
        X = coords[b].reshape(N, 3).astype(F32)
        g = grad[b].reshape(C, N).astype(F32)
        recs = []
        for v in range(V):
            P = proj[b, v].astype(F32).ravel()
            row = lambda r: _fma(P[4 * r + 3], F32(1), _fma(P[4 * r + 2], X[:, 2], _fma(P[4 * r + 1], X[:, 1], P[4 * r] * X[:, 0])))
            a, bb, z = row(0), row(1), row(2)
            front = z > 0
            zs = np.where(front, z, F32(1))
            u, w = a / zs, bb / zs
            ix = ((F32(2) * (u / F32(H) - F32(0.5)) + F32(1)) * F32(0.5)) * F32(W - 1)
            iy = ((F32(2) * (w / F32(W) - F32(0.5)) + F32(1)) * F32(0.5)) * F32(H - 1)
            assert ix.dtype == F32 and iy.dtype == F32
            valid = front & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
            fx0, fy0 = np.where(valid, np.floor(ix), F32(0)), np.where(valid, np.floor(iy), F32(0))
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            x1, y1 = x0 + 1, y0 + 1
            ixv, iyv = np.where(valid, ix, F32(0)), np.where(valid, iy, F32(0))
            wx1, wx0 = ixv - fx0, (fx0 + F32(1)) - ixv
            wy1, wy0 = iyv - fy0, (fy0 + F32(1)) - iyv
            xin0, yin0, yin1 = x0 >= 0, y0 >= 0, y1 <= H - 1
            xin1 = x1 < W - 1 if slip == "x1_lt" else x1 <= W - 1
            xc0, xc1 = np.where(xin0, x0, 0), np.where(xin1, x1, W - 1)
            yc0, yc1 = np.where(yin0, y0, 0), np.where(yin1, y1, H - 1)
            fm = feats[b, v].astype(F32)
            vals, wts = [], []
            for (yc, yin, wy), (xc, xin, wx) in (((yc0, yin0, wy0), (xc0, xin0, wx0)), ((yc0, yin0, wy0), (xc1, xin1, wx1)),
                                                 ((yc1, yin1, wy1), (xc0, xin0, wx0)), ((yc1, yin1, wy1), (xc1, xin1, wx1))):
                inside = xin & yin
                val = fm[:, yc, xc]
                vals.append(val if slip == "no_value_mask" else np.where(inside[None], val, F32(0)))
                wts.append(np.where(inside, wx * wy, F32(0)))
            a00, a01, a10, a11 = vals
            s = _fma(a11, wts[3], _fma(a10, wts[2], _fma(a01, wts[1], a00 * wts[0])))
            dx = _fma(wy0, a01 - a00, wy1 * (a11 - a10))
            dy = _fma(wx0, a10 - a00, wx1 * (a11 - a01))
            m = valid[None]
            recs.append(dict(s=np.where(m, s, F32(0)), dx=np.where(m, dx, F32(0)), dy=np.where(m, dy, F32(0)), valid=valid, z=zs, u=u, w=w, P=P))
        S = np.stack([r["s"] for r in recs])
        if method == "sum":
            ds = np.broadcast_to(g[None], S.shape)
        elif method == "mean":
            ds = np.broadcast_to((g / F32(V))[None], S.shape)
        else:
            am = np.zeros(S.shape[1:], np.int64)
            for v in range(1, V):
                am = np.where(S[v] > np.take_along_axis(S, am[None], 0)[0], v, am)
            ds = np.where(np.arange(V)[:, None, None] == am[None], g[None], F32(0))
        g0 = np.zeros((N, 3), F32)
        order = rng.permutation(N)
        for v in range(V):
            r = recs[v]
            Gx, Gy = np.zeros(N, F32), np.zeros(N, F32)
            for c in range(C):
                Gx, Gy = _fma(ds[v, c], r["dx"][c], Gx), _fma(ds[v, c], r["dy"][c], Gy)
            du, dw = Gx * kx, Gy * ky
            d = np.stack([du / r["z"], dw / r["z"], -(_fma(du, r["u"], dw * r["w"]) / r["z"])], 1)
            d = np.where(r["valid"][:, None], d, F32(0))
            assert d.dtype == F32
            P = r["P"]
            for k in range(3):
                g0[:, k] = _fma(P[8 + k], d[:, 2], _fma(P[4 + k], d[:, 1], _fma(P[k], d[:, 0], g0[:, k])))
            Xh = np.concatenate([X, np.ones((N, 1), F32)], 1)
            for n in order:
                gp[b, v] = _fma(d[n][:, None], Xh[n][None, :], gp[b, v])
        gc[b] = g0
    return gp, gc.reshape((B,) + tuple(vol) + (3,))


def _compared_coords(name, gc):
    """the grad_coords entries a rig compares for the 'not trivially easy' condition: all, or the seeded voxels of a sparse grad_out"""
    seeded = rig.geo_problem(name)[4].get("seeded")
    return gc if seeded is None else gc[:, seeded]


@pytest.mark.parametrize("name", GEO_PLAIN)
def test_geometry_oracles_and_the_fp32_restatement_agree_bit_for_bit(name):
    feats, proj, coords, _, extras = rig.geo_problem(name)
    for method in _geo_methods(name):
        grad, res, _ = rig.geo_reference(name, method)
        gp64, gc64 = geomgrad_oracle.geometry_grad(feats, proj, coords, grad, method)
        assert np.array_equal(gc64, res["grad_coords"]), (name, method, "the two float64 oracles differ in grad_coords")
        if "proj" in extras["want"]:
            assert np.array_equal(gp64, res["grad_proj"]), (name, method, "the two float64 oracles differ in grad_proj")
        for seed in (1, 2):
            gp32, gc32 = _kernel_order32(feats, proj, coords, grad, method, seed)
            assert _same_bits(gc32, res["grad_coords"]), (name, method, "fp32 restatement, grad_coords", seed)
            if "proj" in extras["want"]:
                assert _same_bits(gp32, res["grad_proj"]), (name, method, "fp32 restatement, grad_proj", seed)


def test_cuboid_rig_pose_gradients_agree_with_the_pose_oracle():
    """grad_rot / grad_center of the rig's oracle against tests/posegrad_oracle.py (float64 from fp32 voxel centres): equal exactly; the
    unrotated sample's grad_center is exactly 0, the others' is not"""
    import posegrad_oracle
    feats, proj, coords, _, ex = rig.geo_problem("geo_pose")
    for method in _geo_methods("geo_pose"):
        grad, res, _ = rig.geo_reference("geo_pose", method)
        d32, X32 = posegrad_oracle.cuboid_points(ex["rotations"], ex["centers"], ex["position"], ex["sides"], coords.shape[1:4])
        assert np.array_equal(X32.numpy(), coords) and np.array_equal(d32.numpy().reshape(len(coords), -1, 3), ex["d"])
        gp, gr, gcen = posegrad_oracle.pose_grad(feats, proj, ex["rotations"], ex["centers"], ex["position"], ex["sides"], coords.shape[1:4], grad, method)
        assert np.array_equal(gp, res["grad_proj"]) and np.array_equal(gr, res["grad_rot"]) and np.array_equal(gcen, res["grad_center"])
        assert (res["grad_center"][0] == 0).all() and (res["grad_center"][1:] != 0).any(1).all()
        assert (res["grad_rot"] != 0).mean() >= 0.6


@pytest.mark.parametrize("name", sorted(rig.GEO_RIGS))
def test_geometry_budget_and_difficulty(name):
    feats, proj, coords, _, extras = rig.geo_problem(name) if "M" not in rig.GEO_RIGS[name] else (None,) * 4 + (dict(want=()),)
    if feats is None:                                                # the shared rig is read through its option case alone
        tags = [t[0] for t in rig.geo_option_cases() if t[1] == name]
        for tag in tags:
            res = rig.geo_option_reference(tag)
            assert 0 < res["geo_budget"] < rig.LIMIT
            assert (res["grad_proj"] != 0).mean() >= 0.6 * 3 / 4, (tag, "one of the four samples is named by no volume")
            assert (res["grad_coords"][[0, 1, 2, 4]] != 0).mean() >= 0.6, tag
        return
    for method in _geo_methods(name):
        _, res, ties = rig.geo_reference(name, method)
        rig.assert_geo_budget(res, "%s %s" % (name, method))
        assert 0 < res["geo_budget"] < rig.LIMIT
        assert (_compared_coords(name, res["grad_coords"]) != 0).mean() >= 0.6, (name, method)
        if "proj" in extras["want"]:
            assert (res["grad_proj"] != 0).mean() >= 0.6, (name, method)
        assert ties <= 0.15, (name, method, ties)


def test_geometry_rigs_cover_every_border_condition_between_them():
    total = dict.fromkeys(rig.GEO_STATS, 0)
    for name in GEO_PLAIN:
        st = rig.geo_reference(name, "sum")[1]["stats"]
        for k in total:
            total[k] += st[k]
    for key in ("ix_lo", "ix_hi", "iy_lo", "iy_hi", "ix0", "ixW", "iy0", "iyH", "behind", "z0"):
        assert total[key] > 0, (key, total)


def test_geometry_option_rigs_keep_their_budget():
    for tag, name, method, kw in rig.geo_option_cases():
        res = rig.geo_option_reference(tag)
        rig.assert_geo_budget(res, tag)
        assert (res["grad_coords"] != 0).any() and (res["grad_proj"] != 0).any(), tag


@pytest.mark.parametrize("slip", ["x1_lt", "no_value_mask", "swap_k"])
def test_the_rigs_see_a_slip_in_the_restatement(slip):
    """each deliberate mistake changes bits of grad_coords AND of grad_proj on geo_v3 (a non-square map, so kx != ky), though it stays
    under the 1e-4-of-the-maximum bar for grad_proj that the smooth-data tests apply"""
    feats, proj, coords, _, _ = rig.geo_problem("geo_v3")
    grad, res, _ = rig.geo_reference("geo_v3", "sum")
    gp32, gc32 = _kernel_order32(feats, proj, coords, grad, "sum", 1, slip=slip)
    assert not _same_bits(gc32, res["grad_coords"]) and not _same_bits(gp32, res["grad_proj"]), slip
