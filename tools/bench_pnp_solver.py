#!/usr/bin/env python3
"""Device time of the batched PnPsolver (Tracking::Relocalization: one lost frame against its candidate KeyFrames)
beside the same work in the CPU lane (orbm_pnp_solve_host, the kernels' code on one core), in one run.

  python tools/bench_pnp_solver.py [--solvers 1,8,64] [--matches 100] [--steps 500]

Reports, from HIP events over back-to-back launches on the launch stream with the inputs resident: the setup (the
constructor of every solver), setup + one Relocalization round (iterate with nit = 5 at Tracking's parameters, which
walks to mRansacMaxIts = 35 unless Refine() succeeds first) and setup + find (nit = 300).  Every call evaluates all
the hypotheses of the call whatever the sequential rule then keeps, on the device and in the CPU lane alike.
The scene is synthetic: `matches` BoW matches per candidate, a fifth of them wrong, half a pixel of noise.
Prints one JSON object.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
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


def build(ns, n, seed=0):
    """One frame and ns candidate KeyFrames at stride n: candidate c's MapPoints start at c * n, its feature perm[i]
    holds the point frame feature i sees; the last fifth of every candidate's matches is wrong."""
    rng = np.random.default_rng(seed)
    R, t = rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
    kps = np.zeros((1, n), orbx.KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 4, (1, n))
    d = rng.uniform(5.0, 30.0, n)
    u, v = rng.uniform(30, BOUNDS[1] - 30, n), rng.uniform(30, BOUNDS[3] - 30, n)
    kps["x"][0], kps["y"][0] = u + rng.normal(0, 0.5, n), v + rng.normal(0, 0.5, n)
    Xc = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
    Xw = (Xc - t) @ R
    pts = np.zeros(ns * n, orbx.MAP_POINT_DTYPE)
    pts["flags"] = 3
    kf_mp = np.zeros((ns, n), np.int32)
    match = np.zeros((ns, n), np.int32)
    for c in range(ns):
        lo = c * n
        pts["x"][lo:lo + n], pts["y"][lo:lo + n], pts["z"][lo:lo + n] = Xw.T
        perm = rng.permutation(n)
        kf_mp[c, perm] = lo + np.arange(n)
        match[c] = perm
        wrong = n // 5
        match[c, n - wrong:] = np.roll(match[c, n - wrong:], 1)
    return dict(kps=kps, counts=np.full(1, n, np.int32), kf_mp=kf_mp, pts=pts, match=match)


def one(ns, n, steps, warmup, dev, s):
    w = build(ns, n)
    P = orbx.pose_params(K, BOUNDS, SCALE)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    sv = orbx.PnPsolver(ns, n, 300, P, dev, **orbx.PNP_TRACKING)
    tabs = (T(w["kps"].view(np.int32).reshape(1, n, 7)), T(w["counts"]), T(w["kf_mp"]),
            T(w["pts"].view(np.int32).reshape(-1, 12)), torch.zeros((ns,), dtype=torch.int32, device=dev),
            torch.arange(ns, dtype=torch.int32, device=dev), T(w["match"]))
    rand = np.random.default_rng(1).integers(0, 2 ** 31, (ns, 1200)).astype(np.int32)
    d_rand, d_off = T(rand), torch.arange(ns, dtype=torch.int32, device=dev) * 1200
    out = {"solvers": ns, "setup_ms": round(dev_time(lambda: sv.setup(*tabs, stream=s), steps, warmup, s) * 1e3, 4)}

    def run(nit):
        sv.setup(*tabs, stream=s)
        sv.iterate(nit, d_rand, d_off, stream=s)

    prm = orbx.PoseParams.from_buffer_copy(P)
    nbytes = orbx.lib.orbm_pnp_state_bytes(n)
    p = lambda x, off=0: x.ctypes.data + off   # noqa: E731
    keep = []
    for c in range(ns):
        keep.append(dict(k=w["kps"][0].copy(), km=w["kf_mp"][c].copy(), m=w["match"][c].copy(), rd=rand[c].copy(),
                         st=np.zeros(16, np.int32), state=np.zeros((nbytes + 7) // 8, np.int64),
                         tcw=np.zeros(12, np.float32), inl=np.zeros(n, np.uint8), fmp=np.zeros(n, np.int32)))

    def lane(a, nit):
        a["st"][:2] = 0                                            # a new solver each time
        return orbx.lib.orbm_pnp_solve_host(
            p(a["k"]), n, p(a["km"]), n, p(w["pts"]), len(w["pts"]), p(a["m"]), C.byref(prm), 5.991, 0.99, 10, 300, 4,
            0.5, nit, p(a["rd"]), p(a["st"]), p(a["st"], 4), p(a["state"]), p(a["st"], 8), p(a["tcw"]),
            p(a["st"], 12), p(a["inl"]), p(a["st"], 16), p(a["st"], 20), p(a["st"], 24), p(a["fmp"]), p(a["st"], 28),
            None, 0, None)

    for nit, key in ((5, "round_nit5"), (300, "find_nit300")):
        out[key + "_ms"] = round(dev_time(lambda: run(nit), steps, warmup, s) * 1e3, 4)
        out[key + "_used_mean"] = float(sv.used.float().mean())
        out[key + "_ninliers_mean"] = float(sv.ninliers.float().mean())
        reps = max(1, steps // 50)
        t0 = time.perf_counter()
        for _ in range(reps):
            for a in keep:
                assert lane(a, nit) == orbx.OK
        out[key + "_cpu_lane_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 4)
        out[key + "_cpu_lane_ninliers_mean"] = float(np.mean([a["st"][4] for a in keep]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solvers", default="1,8,64")
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    rows = [one(int(ns), args.matches, args.steps, args.warmup, dev, s) for ns in args.solvers.split(",")]
    print(json.dumps({"bench": "PnPsolver batch", "matches": args.matches, "steps": args.steps, "rows": rows}),
          flush=True)


if __name__ == "__main__":
    main()
