#!/usr/bin/env python3
"""Device time of the batched Frame tail (UndistortKeyPoints, ComputeStereoFromRGBD, isInFrustum) next to the
host round trip each call replaces, in one run, from HIP events over back-to-back launches on the launch
stream with the inputs resident.

  python tools/bench_frame_tail.py [--frames 1024] [--keypoints 2016] [--pframes 64] [--points 4000] [--steps 200]

The keypoint calls run on `frames` x `keypoints` (a TUM1 camera, 640 x 480 depth images); isInFrustum on
`pframes` x `points` MapPoints, about half of them in view.  The round trips copy the same arrays between
device memory and pinned host memory with hipMemcpyAsync on the same stream, timed the same way:
  undistort   keypoints D2H, undistorted keypoints H2D
  rgbd        keypoints and undistorted keypoints D2H, mvuRight and mvDepth H2D (the depth images, which a
              host ComputeStereoFromRGBD would need too, are left out)
  frustum     the packed orbm_proj_point array H2D (the MapPoints live on the host in the reference)
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

TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104,
            p1=-0.005358, p2=0.002628, k3=1.163314)      # Examples/RGB-D/TUM1.yaml
ROWS, COLS, BF = 480, 640, 40.0
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


def keypoints(rng, B, n):
    kps = np.zeros((B, n), orbx.KEYPOINT_DTYPE)
    lvl = rng.integers(0, 8, (B, n))
    sc = np.asarray(SCALE, np.float32)[lvl]
    kps["x"] = (rng.integers(0, (COLS / sc).astype(np.int64)) * sc).astype(np.float32)
    kps["y"] = (rng.integers(0, (ROWS / sc).astype(np.int64)) * sc).astype(np.float32)
    kps["size"], kps["octave"], kps["class_id"] = np.float32(31) * sc, lvl, -1
    return kps


def map_points(rng, B, n):
    K = (TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])
    pts = np.zeros((B, n), orbx.MAP_POINT_DTYPE)
    pose = np.zeros((B, 12), np.float32)
    for f in range(B):
        R, t = rodrigues(rng.normal(0, 0.15, 3)), rng.normal(0, 0.5, 3)
        pose[f] = np.hstack([R, t[:, None]]).ravel()
        u, v = rng.uniform(-200, COLS + 200, n), rng.uniform(-150, ROWS + 150, n)   # ~half inside the image
        d = rng.uniform(2.0, 30.0, n)
        Xc = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
        Xw = (Xc - t) @ R
        PO = Xw + R.T @ t
        dist = np.linalg.norm(PO, axis=1)
        pts["x"][f], pts["y"][f], pts["z"][f] = Xw.T
        pts["nx"][f], pts["ny"][f], pts["nz"][f] = (PO / dist[:, None]).T
        pts["max_dist"][f] = dist * 1.2 ** rng.uniform(0.05, 6.95, n)
        pts["min_dist"][f] = pts["max_dist"][f] / SCALE[7]
        pts["flags"][f] = 3
    return pts, pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--keypoints", type=int, default=2016)
    ap.add_argument("--pframes", type=int, default=64)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    rng = np.random.default_rng(0)
    B, n, PB, pn = args.frames, args.keypoints, args.pframes, args.points
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def pin(t):   # a pinned host copy
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t)
        return h
    t_of = lambda fn: round(dev_time(fn, args.steps, args.warmup, s) * 1e3, 4)
    out = {"bench": "Frame tail batch", "frames": B, "keypoints": n, "pframes": PB, "points": pn, "steps": args.steps}

    cam = orbx.camera(**TUM1)
    kps = T(keypoints(rng, B, n).view(np.int32).reshape(B, n, 7))
    counts = torch.full((B,), n, dtype=torch.int32, device=dev)
    kun = torch.empty_like(kps)
    out["undistort_ms"] = t_of(lambda: orbx.undistort_batch_device(kps, counts, cam, out=kun, stream=s))
    hk, hku = pin(kps), pin(kun)

    def trip_undistort():
        hk.copy_(kps, non_blocking=True)
        kun.copy_(hku, non_blocking=True)
    out["undistort_roundtrip_ms"] = t_of(trip_undistort)

    depth = torch.rand((B, ROWS, COLS), dtype=torch.float32, device=dev) * 8.0
    depth[depth < 0.8] = 0.0                                   # ~10% without depth
    ur = torch.empty((B, n), dtype=torch.float32, device=dev)
    dp = torch.empty((B, n), dtype=torch.float32, device=dev)
    out["rgbd_stereo_ms"] = t_of(lambda: orbx.rgbd_stereo_batch_device(kps, kun, counts, depth, BF, uright=ur,
                                                                       depth_out=dp, stream=s))
    out["rgbd_with_depth_frac"] = round(float((dp > 0).float().mean()), 4)
    hur, hdp = pin(ur), pin(dp)

    def trip_rgbd():
        hk.copy_(kps, non_blocking=True)
        hku.copy_(kun, non_blocking=True)
        ur.copy_(hur, non_blocking=True)
        dp.copy_(hdp, non_blocking=True)
    out["rgbd_roundtrip_ms"] = t_of(trip_rgbd)
    del depth

    hp, hpose = map_points(rng, PB, pn)
    pts, pose = T(hp.view(np.int32).reshape(PB, pn, 12)), T(hpose)
    npts = torch.full((PB,), pn, dtype=torch.int32, device=dev)
    bounds = orbx.image_bounds(cam, ROWS, COLS)
    pp = orbx.pose_params((TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"]), bounds, SCALE, bf=BF)
    proj = torch.empty((PB, pn, 6), dtype=torch.int32, device=dev)
    nv = torch.empty((PB,), dtype=torch.int32, device=dev)
    out["frustum_ms"] = t_of(lambda: orbx.frustum_batch_device(pts, npts, pose, pp, 0.5, out=proj, ninview=nv,
                                                               stream=s))
    out["frustum_inview_frac"] = round(float(nv.float().mean()) / pn, 4)
    hproj = pin(proj)
    out["frustum_upload_ms"] = t_of(lambda: proj.copy_(hproj, non_blocking=True))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
