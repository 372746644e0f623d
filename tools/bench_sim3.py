#!/usr/bin/env python3
"""Device time of the batched SearchBySim3 (LoopClosing::ComputeSim3: one current KeyFrame against its loop
candidates) next to Fuse(KF, Scw) on the same KeyFrames and MapPoints, in one run, from HIP events over
back-to-back launches on the launch stream with the inputs resident.

  python tools/bench_sim3.py [--candidates 32] [--features 2000] [--steps 200]

The scene is synthetic: `features` physical points seen by KF0 and, through a Sim3 (s12 = 1.7, a small rotation
and translation), by every candidate; a feature per visible point plus noise, clustered descriptors, MapPoint
distance ranges that predict the feature's octave or the next.  Fuse gets KF0's MapPoints projected into each
candidate with Scw = S21 * T0w, once at SearchAndFuse's th = 4 and once at SearchBySim3's 7.5.
Prints one JSON object.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbx  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)   # Examples/Stereo/KITTI00-02.yaml
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
SCALE = [np.float32(1.2) ** i for i in range(8)]


def dev_time(fn, steps, warmup, stream):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e-3


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def flip(rng, src, p):
    return np.packbits(np.unpackbits(src, axis=-1) ^ (rng.random(src.shape[:-1] + (256,)) < p), axis=-1)


def build(ncand, n, s12, seed=0):
    rng = np.random.default_rng(seed)
    B = ncand + 1
    proto = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    owner = rng.integers(0, 64, n)
    octave = rng.integers(0, 7, n)
    depth = rng.uniform(5.0, 30.0, n)
    u0, v0 = rng.uniform(30, BOUNDS[1] - 30, n), rng.uniform(30, BOUNDS[3] - 30, n)
    pc = [np.stack([(u0 - K[2]) / K[0] * depth, (v0 - K[3]) / K[1] * depth, depth], 1)]
    pose = [np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))])]
    sim3 = np.zeros((ncand, 13), np.float32)
    scw = np.zeros((ncand, 24), np.float32)
    for k in range(ncand):
        R12, t12 = rodrigues(rng.normal(0, 0.03, 3)), rng.normal(0, 0.2, 3)
        sim3[k] = np.concatenate([[s12], R12.ravel(), t12])
        pc.append((pc[0] - t12) @ R12 / s12)                            # (1/s) R12^T (pc0 - t12)
        pose.append(np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))]))
        sR21 = R12.T / s12
        scw[k, :12] = np.hstack([sR21 @ pose[0][:, :3], (sR21 @ pose[0][:, 3] - sR21 @ t12)[:, None]]).ravel()
    kps = np.zeros((B, n), orbx.KEYPOINT_DTYPE)
    mps = np.zeros((B, n), orbx.MAP_POINT_DTYPE)
    desc = np.zeros((B, n, 32), np.uint8)
    mpdesc = np.zeros((B, n, 32), np.uint8)
    for f in range(B):
        u = K[0] * pc[f][:, 0] / pc[f][:, 2] + K[2] + rng.normal(0, 1, n)
        v = K[1] * pc[f][:, 1] / pc[f][:, 2] + K[3] + rng.normal(0, 1, n)
        out = (u < 1) | (u > BOUNDS[1] - 2) | (v < 1) | (v > BOUNDS[3] - 2)
        kps["x"][f] = np.where(out, rng.uniform(1, BOUNDS[1] - 2, n), u)
        kps["y"][f] = np.where(out, rng.uniform(1, BOUNDS[3] - 2, n), v)
        kps["octave"][f] = octave
        desc[f], mpdesc[f] = flip(rng, proto[owner], 0.05), flip(rng, proto[owner], 0.06)
        R, t = pose[f][:, :3], pose[f][:, 3]
        Xw = (pc[f] - t) @ R
        other = pc[1] if f == 0 else pc[0]                              # KF0's ranges fit candidate 1's view
        mps["x"][f], mps["y"][f], mps["z"][f] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
        mps["max_dist"][f] = np.linalg.norm(other, axis=1) * 1.2 ** (octave + rng.uniform(0.05, 0.95, n))
        mps["min_dist"][f] = mps["max_dist"][f] / SCALE[7]
        mps["flags"][f] = rng.random(n) < 0.9
    # Fuse(candidate k, Scw, KF0's MapPoints): the distance test is on |P - Ow| in world units, s12 * |pc_k|
    fpts = np.repeat(mps[0][None], ncand, 0)
    for k in range(ncand):
        Ow = pose[0][:, :3].T @ (sim3[k, 10:13].astype(np.float64) - pose[0][:, 3])   # camera k's centre in KF0's world
        PO = np.stack([mps["x"][0], mps["y"][0], mps["z"][0]], 1) - Ow
        d = np.linalg.norm(PO, axis=1)
        fpts["nx"][k], fpts["ny"][k], fpts["nz"][k] = (PO / d[:, None]).T
        fpts["max_dist"][k] = d * 1.2 ** (octave + rng.uniform(0.05, 0.95, n))
        fpts["min_dist"][k] = fpts["max_dist"][k] / SCALE[7]
    return dict(kps=kps, desc=desc, mps=mps, mpdesc=mpdesc, pose=np.stack(pose).reshape(B, 12).astype(np.float32),
                sim3=sim3, scw=scw, fpts=fpts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    nc, n = args.candidates, args.features
    w = build(nc, n, 1.7)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kps, desc = T(w["kps"].view(np.int32).reshape(nc + 1, n, 7)), T(w["desc"])
    mps, mpdesc = T(w["mps"].view(np.int32).reshape(nc + 1, n, 12)), T(w["mpdesc"])
    counts = torch.full((nc + 1,), n, dtype=torch.int32, device=dev)
    pa = torch.zeros((nc,), dtype=torch.int32, device=dev)
    pb = torch.arange(1, nc + 1, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(1)
    al1, al2 = T((rng.random((nc, n)) < 0.1).astype(np.uint8)), T((rng.random((nc, n)) < 0.1).astype(np.uint8))
    pose, sim3 = T(w["pose"]), T(w["sim3"])
    mt = orbx.ORBmatcher(0.9, True)
    pp = lambda th: orbx.pose_params(K, BOUNDS, SCALE, th=th)
    m12 = torch.empty((nc, n), dtype=torch.int32, device=dev)
    nf = torch.empty((nc,), dtype=torch.int32, device=dev)
    p75 = pp(7.5)
    t_s3 = dev_time(lambda: mt.search_by_sim3_batch_device(kps, desc, mps, mpdesc, counts, pose, pa, pb, sim3, al1, al2,
                                                           p75, match12=m12, nfound=nf, stream=s),
                    args.steps, args.warmup, s)
    out = {"bench": "SearchBySim3 batch", "pairs": nc, "features": n, "steps": args.steps,
           "search_by_sim3_ms": round(t_s3 * 1e3, 4), "nfound_mean": float(nf.float().mean())}
    # Fuse(KF, Scw) over the candidates: their keypoints, KF0's MapPoints
    fpts, fdesc = T(w["fpts"].view(np.int32).reshape(nc, n, 12)), mpdesc[0:1].expand(nc, n, 32).contiguous()
    ur = torch.full((nc, n), -1.0, dtype=torch.float32, device=dev)
    cl = torch.zeros((nc, n), dtype=torch.uint8, device=dev)
    npts = torch.full((nc,), n, dtype=torch.int32, device=dev)
    scw = T(w["scw"])
    fm = torch.empty((nc, n), dtype=torch.int32, device=dev)
    fn = torch.empty((nc,), dtype=torch.int32, device=dev)
    for th in (4.0, 7.5):
        prm = pp(th)
        t = dev_time(lambda: mt.project_search_batch_device(orbx.FUSE_SIM3, kps[1:], desc[1:], ur, cl, counts[1:], scw,
                                                            fpts, fdesc, npts, prm, match=fm, nmatches=fn, stream=s),
                     args.steps, args.warmup, s)
        out["fuse_sim3_th%g_ms" % th] = round(t * 1e3, 4)
        out["fuse_sim3_th%g_nfused_mean" % th] = float(fn.float().mean())
        out["ratio_to_fuse_th%g" % th] = round(t_s3 / t, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
