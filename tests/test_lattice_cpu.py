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
