#!/usr/bin/env python3
"""Device time of one MapPoint refresh (ComputeDistinctiveDescriptors + UpdateNormalAndDepth over a KeyFrame table),
from HIP events over back-to-back launches on the launch stream with the inputs resident, at three sizes:

  local   2,000 MapPoints x ~8 observations   (the MapPoints of one new KeyFrame, LocalMapping::ProcessNewKeyFrame)
  global  20,000 MapPoints x ~15 observations (a whole map after a global bundle adjustment)
  long    2,000 MapPoints x ~33 observations  (half of them above 32 good rows, where the kernel's median leaves
                                               the registers for passes over LDS)

  python tools/bench_map_points.py [--steps 200] [--keyframes 64] [--features 2000]

For scale, the same work in a single-thread numpy loop on the host (one MapPoint at a time: the N x N popcount
table, a sort per row, the unit vectors), timed once.  It is a yardstick for the order of magnitude, not the
reference's C++.  Prints one JSON object per size.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbx  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)   # Examples/Stereo/KITTI00-02.yaml
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
SCALE = [np.float32(1.2) ** i for i in range(8)]
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


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


def build(nkf, nfeat, npts, mean_obs, seed=0):
    """A table of nkf KeyFrames x nfeat features with clustered descriptors, and npts MapPoints seen by
    2 .. 2 * mean_obs - 2 distinct KeyFrames each (ascending, as a std::map of KeyFrame pointers would iterate)."""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    kps = np.zeros((nkf, nfeat), orbx.KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 8, (nkf, nfeat))
    desc = rng.integers(0, 256, (nkf, nfeat, 32), dtype=np.uint8)
    pose = np.zeros((nkf, 12), np.float32)
    for f in range(nkf):
        a = rng.normal(0, 0.2)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        pose[f] = np.hstack([R, rng.normal(0, 2.0, (3, 1))]).ravel()
    lens = rng.integers(2, min(nkf, 2 * mean_obs - 2) + 1, npts)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    obs = np.zeros(ptr[-1], orbx.OBSERVATION_DTYPE)
    ref = np.zeros(npts, orbx.OBSERVATION_DTYPE)
    for m in range(npts):
        kfs = np.sort(rng.choice(nkf, lens[m], replace=False))
        idx = rng.integers(0, nfeat, lens[m])
        obs["kf"][ptr[m]:ptr[m + 1]], obs["idx"][ptr[m]:ptr[m + 1]] = kfs, idx
        noise = rng.random((lens[m], 256)) < 0.06
        desc[kfs, idx] = np.packbits(np.unpackbits(proto[m])[None] ^ noise, axis=1)
        ref[m] = (kfs[0], idx[0])
    pts = np.zeros(npts, orbx.MAP_POINT_DTYPE)
    xyz = rng.normal(0, 1.0, (npts, 3)) * (10, 3, 10) + (0, 0, 25)
    pts["x"], pts["y"], pts["z"] = xyz.T.astype(np.float32)
    pts["flags"] = 3
    bad = (rng.random(nkf) < 0.05).astype(np.uint8)
    return dict(kps=kps, desc=desc, counts=np.full(nkf, nfeat, np.int32), pose=pose, bad=bad, ptr=ptr, obs=obs, ref=ref,
                pts=pts, max_obs=int(lens.max()), mean_obs=float(lens.mean()))


def host_loop(w):
    """One MapPoint at a time in numpy, single thread: returns (seconds, winners)."""
    Ow = np.stack([-(p.reshape(3, 4)[:, :3].T @ p.reshape(3, 4)[:, 3]) for p in w["pose"]])
    xyz = np.stack([w["pts"]["x"], w["pts"]["y"], w["pts"]["z"]], 1)
    scale = np.array(SCALE, np.float32)
    best = np.full(len(w["pts"]), -1, np.int32)
    t0 = time.perf_counter()
    for m in range(len(best)):
        o = w["obs"][w["ptr"][m]:w["ptr"][m + 1]]
        v = xyz[m] - Ow[o["kf"]]
        normal = (v / np.linalg.norm(v, axis=1)[:, None]).sum(0) / len(o)
        d = np.linalg.norm(xyz[m] - Ow[w["ref"]["kf"][m]]) * scale[w["kps"]["octave"][w["ref"]["kf"][m], w["ref"]["idx"][m]]]
        good = np.nonzero(w["bad"][o["kf"]] == 0)[0]
        if len(good):
            D = w["desc"][o["kf"][good], o["idx"][good]]
            dm = POPCOUNT[D[:, None, :] ^ D[None, :, :]].sum(2)
            med = np.sort(dm, axis=1)[:, (len(good) - 1) // 2]
            best[m] = good[np.argmin(med)]
    return time.perf_counter() - t0, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true", help="skip the host numpy loop")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pp = orbx.pose_params(K, BOUNDS, SCALE)
    for name, npts, mean_obs in (("local", 2000, 8), ("global", 20000, 15), ("long", 2000, 33)):
        w = build(args.keyframes, args.features, npts, mean_obs)
        nkf, nfeat = w["kps"].shape
        kps, desc = T(w["kps"].view(np.int32).reshape(nkf, nfeat, 7)), T(w["desc"])
        counts, pose, bad = T(w["counts"]), T(w["pose"]), T(w["bad"])
        ptr, obs = T(w["ptr"]), T(w["obs"].view(np.int32).reshape(-1, 2))
        ref = T(w["ref"].view(np.int32).reshape(-1, 2))
        pts, pdesc = T(w["pts"].view(np.int32).reshape(npts, 12)), torch.zeros((npts, 32), dtype=torch.uint8, device=dev)
        best = torch.empty((npts,), dtype=torch.int32, device=dev)
        out = {"bench": "MapPoint refresh", "size": name, "points": npts, "mean_obs": round(w["mean_obs"], 2),
               "max_obs": w["max_obs"], "keyframes": nkf, "features": nfeat, "steps": args.steps}
        for key, what in (("descriptor_ms", 1), ("normal_depth_ms", 2), ("both_ms", 3)):
            t = dev_time(lambda: orbx.refresh_map_points_device(what, kps, desc, counts, pose, bad, ptr, obs, ref,
                                                                w["max_obs"], pp, pts, pdesc, best=best, stream=s),
                         args.steps, args.warmup, s)
            out[key] = round(t * 1e3, 4)
        if not args.no_host:
            th, hbest = host_loop(w)
            out["host_numpy_loop_ms"] = round(th * 1e3, 1)
            out["winners_agree"] = bool(np.array_equal(hbest, best.cpu().numpy()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
