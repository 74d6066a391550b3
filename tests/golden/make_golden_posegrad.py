#!/usr/bin/env python3
"""Generate tests/golden/posegrad_<case>.npz by RUNNING the reference's VolumeGenerator(use_triangulation=True) with proj_matricies and
the features requiring grad: autograd reaches proj_matricies through the triangulated pivot (torch.svd, fp32) and the rotated cuboid
coordinates, as the reference's graph has it.  Also one case of the reference's triangulate_point_from_multiple_views_linear_torch
alone, per sample, with confidences and points requiring grad.

Run it only where the reference code base is importable, like make_golden.py (whose synthetic cameras and batch construction it
reuses; importing it imports the reference).  CPU only.  Besides the reference's gradients every VolumeGenerator file holds the float64
oracle's proj_matricies gradient (tests/posegrad_oracle.py) for the same inputs: the distance between the two is the reference's own fp32
error, from which the GPU test sets its bound.  It is mostly the error of the reference's fp32 pivot (stored as ref_center): at that
pivot the oracle and the reference agree closely (tests/test_pose_grad_cpu.py).

Usage:  python tests/golden/make_golden_posegrad.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: the oracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root: oracle.reference_loop_torch

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (imports the reference)
from posegrad_oracle import dlt_grad, pose_grad  # noqa: E402


def _cameras(B, V, image_hw, rng):
    """run_volgen_case's rig: a jittered ring, per-sample translation noise, crop then resize"""
    cams = mg.ring_cameras(V, 5000.0, 1500.0, 1145.0, 1000.0, rng, jitter=0.04)
    bbox = (150, 150, 850, 850)
    Ks, Rs, ts, cameras = [], [], [], []
    for v in range(V):
        row = []
        for b in range(B):
            R, t, K = cams[v]
            cam = mg.ref_mv.Camera(R, t + rng.normal(0, 5.0, 3), K)
            cam.update_after_crop(bbox)
            cam.update_after_resize((700, 700), (image_hw[1], image_hw[0]))
            row.append(cam)
            Ks.append(cam.K.copy()); Rs.append(cam.R.copy()); ts.append(cam.t.copy())
        cameras.append(row)
    return cameras, np.stack(Ks).reshape(V, B, 3, 3), np.stack(Rs).reshape(V, B, 3, 3), np.stack(ts).reshape(V, B, 3, 1)


def run_case(name, *, B, V, C_in, C_out, S, feat_hw, image_hw, kind, training, seed, method="softmax"):
    rng = np.random.default_rng(seed)
    cameras, K, R, t = _cameras(B, V, image_hw, rng)
    keypoints = [rng.normal(0, 100.0, (17, 4)) for _ in range(B)]
    batch = dict(images=np.zeros((B, V, image_hw[0], image_hw[1], 3), dtype=np.uint8), cameras=cameras, keypoints_3d=keypoints)
    torch.manual_seed(seed)
    gen = mg.ref_agg.VolumeGenerator(volume_size=S, input_channels=C_in, output_channels=C_out, cuboid_side=2500.0,
                                     aggregation_method=method, use_triangulation=True, kind=kind, device="cpu")
    gen.train(training)
    features = torch.randn(B, V, C_in, *feat_hw)
    proj_org = torch.stack([torch.stack([torch.from_numpy(cameras[v][b].projection) for v in range(V)]) for b in range(B)]).float()
    grad_out = torch.randn(B, C_out, S, S, S, generator=torch.Generator().manual_seed(seed + 3000))
    captured = {}
    real = mg.ref_agg.unprojection

    def spy(f, p, c, aggregation_method="softmax"):
        captured.update(features=f.detach().numpy().copy(), proj=p.numpy().copy(), coords=c.detach().numpy().copy())
        return real(f, p, c, aggregation_method=aggregation_method)

    f = features.clone().requires_grad_(True)
    P = proj_org.clone().requires_grad_(True)
    mg.ref_agg.unprojection = spy
    try:
        np.random.seed(seed)
        vol = gen(f, P, batch)
    finally:
        mg.ref_agg.unprojection = real
    (vol * grad_out).sum().backward()
    sd = gen.state_dict()
    conv = gen.process_feature[0]

    # the float64 oracle for the same inputs: the pivot by a float64 DLT, the pose gradient of the cuboid recipe, the DLT's backward
    np.random.seed(seed)
    thetas = [np.random.uniform(0.0, 2 * np.pi) if training else 0.0 for _ in range(B)]
    axis = [0, 1, 0] if kind == "coco" else [0, 0, 1]
    rot = np.stack([mg.ref_vol.get_rotation_matrix(axis, th) for th in thetas]).astype(np.float32)
    uv = (torch.tensor(image_hw) / 2).expand(V, 2).numpy().astype(np.float32)
    P64 = proj_org.double()
    A = P64[:, :, 2:3].expand(B, V, 2, 4) * torch.from_numpy(uv).double().view(1, V, 2, 1) - P64[:, :, :2]
    h = torch.linalg.svd(A.reshape(B, 2 * V, 4), full_matrices=False)[2][:, 3]
    center = (h[:, :3] / h[:, 3:4]).float().numpy()
    side = 2500.0
    position, sides = [-side / 2] * 3, [side] * 3
    _, _, g_center = pose_grad(captured["features"], captured["proj"], rot, center, position, sides, (S, S, S), grad_out.numpy(), method)
    oracle_gproj_org = dlt_grad(proj_org.numpy(), uv, None, g_center)[0]
    # the pivot the reference itself used (fp32 torch.svd, as aggregation.py:174-177 computes it): where the reference and the oracle
    # differ, it is mostly by this pivot's fp32 error moving voxels across cells
    A32 = (proj_org[:, :, 2:3].expand(B, V, 2, 4) * torch.from_numpy(uv).view(1, V, 2, 1) - proj_org[:, :, :2]).reshape(B, 2 * V, 4)
    ref_center = np.stack([(lambda h: (h[:3] / h[3]).numpy())(-torch.svd(A32[b])[2][:, 3]) for b in range(B)]).astype(np.float32)

    rec = dict(K=K, R=R, t=t, keypoints=np.stack(keypoints), image_hw=np.array(image_hw), features_in=features.numpy(),
               proj_org=proj_org.numpy(), weight=sd["process_feature.0.weight"].numpy(), bias=sd["process_feature.0.bias"].numpy(),
               grad_out=grad_out.numpy(), rot=rot, center=center, images_center=uv,
               gproj_org=P.grad.numpy(), gfeatures=f.grad.numpy(), gweight=conv.weight.grad.numpy(), gbias=conv.bias.grad.numpy(),
               oracle_gproj_org=oracle_gproj_org, oracle_gcenter=g_center, ref_center=ref_center, proj=captured["proj"],
               meta=np.array([B, V, C_in, C_out, S, int(training), 1, seed]), kind=np.array(kind), method=np.array(method))
    path = os.path.join(HERE, "posegrad_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote", path, "reference vs float64 oracle (proj_org.grad): %.3e max-abs, scale %.3e"
          % (np.abs(P.grad.numpy() - oracle_gproj_org).max(), np.abs(oracle_gproj_org).max()))


def run_dlt_case(name, *, B, V, seed):
    """the reference's torch DLT per sample, confidences and points (per sample) requiring grad"""
    rng = np.random.default_rng(seed)
    cams = mg.ring_cameras(V, 5000.0, 1500.0, 1145.0, 1000.0, rng, jitter=0.04)
    P = np.stack([np.stack([mg.ref_mv.Camera(Rc, tc + rng.normal(0, 5.0, 3), Kc).projection for Rc, tc, Kc in cams]) for _ in range(B)])
    P = P.astype(np.float32)
    X = rng.uniform(-300, 300, (B, 3))
    hom = np.concatenate([X, np.ones((B, 1))], 1)
    r = np.einsum("bvij,bj->bvi", P.astype(np.float64), hom)
    uv = (r[..., :2] / r[..., 2:3] + rng.normal(0, 2.0, (B, V, 2))).astype(np.float32)
    conf = rng.uniform(0.3, 1.0, (B, V)).astype(np.float32)
    go = rng.standard_normal((B, 3)).astype(np.float32)
    gP, gU, gC, out = [], [], [], []
    for b in range(B):
        Pb = torch.from_numpy(P[b]).clone().requires_grad_(True)
        ub = torch.from_numpy(uv[b]).clone().requires_grad_(True)
        cb = torch.from_numpy(conf[b]).clone().requires_grad_(True)
        x = mg.ref_mv.triangulate_point_from_multiple_views_linear_torch(Pb, ub, cb)
        (x * torch.from_numpy(go[b])).sum().backward()
        gP.append(Pb.grad.numpy()); gU.append(ub.grad.numpy()); gC.append(cb.grad.numpy()); out.append(x.detach().numpy())
    path = os.path.join(HERE, "posegrad_%s.npz" % name)
    np.savez_compressed(path, proj=P, points=uv, confidences=conf, grad_out=go, out=np.stack(out), gproj=np.stack(gP),
                        gpoints=np.stack(gU), gconf=np.stack(gC))
    print("wrote", path)


def main():
    run_case("train_tri_mpii", B=2, V=3, C_in=5, C_out=4, S=6, feat_hw=(12, 16), image_hw=(48, 64), kind="mpii", training=True, seed=31)
    run_case("eval_tri_coco", B=2, V=4, C_in=4, C_out=8, S=5, feat_hw=(16, 32), image_hw=(64, 128), kind="coco", training=False, seed=32)
    # shapes the fused conv + un-projection path (_FusedAggregate) takes: C_in % 16, C_out % 128, Hf % 4, Wf % 32
    run_case("train_tri_fusedshape", B=1, V=3, C_in=16, C_out=128, S=4, feat_hw=(4, 32), image_hw=(16, 128), kind="mpii", training=True,
             seed=34)
    run_dlt_case("dlt_conf_v4", B=3, V=4, seed=33)


if __name__ == "__main__":
    main()
