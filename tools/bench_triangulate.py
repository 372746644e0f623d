#!/usr/bin/env python3
"""Device time of one orbm_triangulate_device call (the match loop of LocalMapping::CreateNewMapPoints: parallax,
4x4 Jacobi SVD or stereo unprojection, the depth / reprojection / scale tests, then the per-pair compaction), from
HIP events over back-to-back calls on the launch stream with the inputs resident, at two sizes:

  insertion  20 pairs x 300 matches     (one new KeyFrame against its 20 covisible neighbours)
  replay     2,000 pairs x 300 matches  (an offline replay batched over 100 KeyFrame insertions)

  python tools/bench_triangulate.py [--steps 200] [--matches 300] [--stereo 0.3]

The call is two kernels, k_triangulate and k_triang_compact; the events time them together.  Their split comes from a
kernel trace, in a run of its own (tracing slows the host):

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_triangulate.py --steps 50

Prints one JSON object per size: the time per call, per pair and per match, and what became of the matches.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbx  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)   # Examples/Stereo/KITTI00-02.yaml
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
BF = 386.1448
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


def build(npairs, nfeat, stereo, seed=0):
    """KeyFrame 0 and npairs neighbours along a KITTI-like forward motion with some sideways drift, all seeing the
    same nfeat points (feature j = point j) with 0.4 px of noise; 85% of the features matched, 3% of the matches
    wrong.  A share `stereo` of the keypoints carries uRight and depth."""
    rng = np.random.default_rng(seed)
    nkf = npairs + 1
    pts = np.stack([rng.uniform(-12, 12, nfeat), rng.uniform(-2, 3, nfeat), rng.uniform(6, 60, nfeat)], 1)
    pose = np.zeros((nkf, 3, 4))
    kps = np.zeros((nkf, nfeat), orbx.KEYPOINT_DTYPE)
    ur = np.full((nkf, nfeat), -1, np.float32)
    dp = np.full((nkf, nfeat), -1, np.float32)
    octave = rng.integers(0, 8, nfeat)
    for f in range(nkf):
        a = rng.normal(0, 0.01) if f else 0.0
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = np.array([rng.normal(0, 0.4), rng.normal(0, 0.05), rng.uniform(-1.5, 1.5)]) if f else np.zeros(3)
        pose[f] = np.hstack([R, (-R @ c)[:, None]])
        x = pts @ R.T + pose[f, :, 3]
        u = K[0] * x[:, 0] / x[:, 2] + K[2] + rng.normal(0, 0.4, nfeat)
        v = K[1] * x[:, 1] / x[:, 2] + K[3] + rng.normal(0, 0.4, nfeat)
        kps["x"][f], kps["y"][f], kps["octave"][f] = u, v, octave
        st = (rng.random(nfeat) < stereo) & (x[:, 2] > 0) & (u - BF / x[:, 2] >= 0)
        ur[f, st] = (u - BF / x[:, 2] + rng.normal(0, 0.3, nfeat))[st]
        dp[f, st] = x[st, 2]
    match = np.tile(np.arange(nfeat, dtype=np.int32), (npairs, 1))
    wrong = rng.random(match.shape) < 0.03
    match[wrong] = rng.integers(0, nfeat, int(wrong.sum()))
    match[rng.random(match.shape) < 0.15] = -1
    return dict(kps=kps, uright=ur, depth=dp, counts=np.full(nkf, nfeat, np.int32),
                pose=pose.reshape(nkf, 12).astype(np.float32), pair_a=np.zeros(npairs, np.int32),
                pair_b=np.arange(1, nkf, dtype=np.int32), match=match)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--stereo", type=float, default=0.3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pp = orbx.pose_params(K, BOUNDS, SCALE, bf=BF)
    names = ("no_match", "svd", "stereo1", "stereo2", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2",
             "zero_dist", "scale", "invalid")
    for name, npairs in (("insertion", 20), ("replay", 2000)):
        w = build(npairs, args.matches, args.stereo)
        nkf, nfeat = w["kps"].shape
        kps = T(w["kps"].view(np.int32).reshape(nkf, nfeat, 7))
        counts, pose, pa, pb, match = T(w["counts"]), T(w["pose"]), T(w["pair_a"]), T(w["pair_b"]), T(w["match"])
        ur, dp = T(w["uright"]), T(w["depth"])
        mark = torch.zeros((nkf, nfeat), dtype=torch.uint8, device=dev)
        out = orbx.triangulate_device(kps, counts, pose, pa, pb, match, pp, uright=ur, depth=dp, mark=mark, stream=s)
        t = dev_time(lambda: orbx.triangulate_device(kps, counts, pose, pa, pb, match, pp, uright=ur, depth=dp,
                                                     mark=mark, out=out, stream=s), args.steps, args.warmup, s)
        st = np.bincount(out["status"].cpu().numpy().ravel(), minlength=13)
        nmatch = int((w["match"] >= 0).sum())
        print(json.dumps({"bench": "triangulate", "size": name, "pairs": npairs, "features": nfeat, "matches": nmatch,
                          "steps": args.steps, "call_ms": round(t * 1e3, 4), "per_pair_us": round(t * 1e6 / npairs, 3),
                          "per_match_ns": round(t * 1e9 / nmatch, 2), "created": int(out["nnew"].sum().item()),
                          "status": {k: int(v) for k, v in zip(names, st) if v}}), flush=True)


if __name__ == "__main__":
    main()
