#!/usr/bin/env python3
"""Device time of the batched Sim3Solver (LoopClosing::ComputeSim3: one current KeyFrame against its loop
candidates) beside the same work in the CPU lane (orbm_sim3_solve_host, the kernels' code on one core), in one run.

  python tools/bench_sim3_solver.py [--candidates 8] [--pairs 150] [--steps 5000]

Reports, from HIP events over back-to-back launches on the launch stream with the inputs resident: the setup (the
constructor of every candidate's solver), one ComputeSim3 round (iterate with nit = 5 for every candidate) and find
(nit = 300).  Every call evaluates all nit hypotheses of every solver whatever the sequential rule then keeps, on
the device and in the CPU lane alike, so the two times are for the same arithmetic.  The state is reset between the
timed calls (two int32 fills of `candidates` words, inside the timed region).
The scene is synthetic: `pairs` BoW matches per candidate, a fifth of them wrong, the MapPoints seen through a Sim3
(s12 = 1.3, a rotation of 0.3 rad, a translation) with half a pixel of noise.
Prints one JSON object.
"""
from __future__ import annotations

import argparse
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


def build(ncand, n, seed=0):
    """KeyFrame 0 (the current one) and ncand candidates at stride n; MapPoints 0..n-1 belong to KeyFrame 0, those
    of candidate c start at (c + 1) * n; every MapPoint is observed by its own feature."""
    rng = np.random.default_rng(seed)
    B = ncand + 1
    pose = lambda: np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))])   # noqa: E731
    back = lambda T, Xc: (Xc - T[:, 3]) @ T[:, :3]                                              # noqa: E731
    d = rng.uniform(5.0, 30.0, n)
    u, v = rng.uniform(30, BOUNDS[1] - 30, n), rng.uniform(30, BOUNDS[3] - 30, n)
    X0 = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
    T = [pose()]
    kps = np.zeros((B, n), orbx.KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 4, (B, n))
    pts = np.zeros(B * n, orbx.MAP_POINT_DTYPE)
    pts["flags"] = 3
    Xw = back(T[0], X0)
    pts["x"][:n], pts["y"][:n], pts["z"][:n] = Xw.T
    match12 = np.zeros((ncand, n), np.int32)
    for c in range(ncand):
        R12, t12 = rodrigues(rng.normal(0, 0.3 / math.sqrt(3), 3)), rng.normal(0, 0.3, 3)
        Xc = (X0 - t12) @ R12 / 1.3
        Xc = Xc + rng.normal(0, 1, (n, 3)) * (0.5 * Xc[:, 2:3] / K[0])
        T.append(pose())
        perm = rng.permutation(n)
        Xw = back(T[-1], Xc)
        lo = (c + 1) * n
        pts["x"][lo + perm], pts["y"][lo + perm], pts["z"][lo + perm] = Xw.T      # feature perm[i] sees point i
        match12[c] = perm
        wrong = n // 5
        match12[c, n - wrong:] = np.roll(match12[c, n - wrong:], 1)
    kf_mp = np.arange(B * n, dtype=np.int32).reshape(B, n)
    obs = np.zeros(B * n, orbx.OBSERVATION_DTYPE)
    obs["kf"], obs["idx"] = np.repeat(np.arange(B), n), np.tile(np.arange(n), B)
    return dict(kps=kps, counts=np.full(B, n, np.int32), pose=np.stack(T).reshape(B, 12).astype(np.float32),
                kf_mp=kf_mp, pts=pts, obs_ptr=np.arange(B * n + 1, dtype=np.int32), obs=obs, match12=match12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    nc, n = args.candidates, args.pairs
    w = build(nc, n)
    P = orbx.pose_params(K, BOUNDS, SCALE)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    sv = orbx.Sim3Solver(nc, n, 300, P, dev)
    pa = torch.zeros((nc,), dtype=torch.int32, device=dev)
    pb = torch.arange(1, nc + 1, dtype=torch.int32, device=dev)
    tabs = (T(w["kps"].view(np.int32).reshape(nc + 1, n, 7)), T(w["counts"]), T(w["pose"]), T(w["kf_mp"]),
            T(w["pts"].view(np.int32).reshape(-1, 12)), T(w["obs_ptr"]), T(w["obs"].view(np.int32).reshape(-1, 2)), pa, pb,
            T(w["match12"]))
    rand = np.random.default_rng(1).integers(0, 2 ** 31, (nc, 900)).astype(np.int32)
    d_rand, d_off = T(rand), torch.arange(nc, dtype=torch.int32, device=dev) * 900
    t_setup = dev_time(lambda: sv.setup(*tabs, stream=s), args.steps, args.warmup, s)

    def iterate(nit):
        sv.iterations.zero_()
        sv.best_inliers.zero_()
        sv.iterate(nit, d_rand, d_off, stream=s)

    out = {"bench": "Sim3Solver batch", "candidates": nc, "pairs": n, "steps": args.steps,
           "setup_ms": round(t_setup * 1e3, 4)}
    # the CPU lane on the same inputs: the argument lists are built once, the timed loop is the C calls alone
    import ctypes as C
    prm = orbx.PoseParams.from_buffer_copy(P)
    keep, lane = [], []
    for c in range(nc):
        ob = w["obs"].copy()                                   # KeyFrame 0 is slot 0, the candidate slot 1
        ob["kf"] = np.where(ob["kf"] == 0, 0, np.where(ob["kf"] == c + 1, 1, 99))
        a = dict(k1=w["kps"][0].copy(), m1=w["kf_mp"][0].copy(), k2=w["kps"][c + 1].copy(), m2=w["kf_mp"][c + 1].copy(),
                 t1=w["pose"][0].copy(), t2=w["pose"][c + 1].copy(), ob=ob, m12=w["match12"][c].copy(), rd=rand[c].copy(),
                 st=np.zeros(8, np.int32), sim3=np.zeros(13, np.float32), i12=np.zeros(n, np.uint8),
                 a2=np.zeros(n, np.uint8))
        keep.append(a)
        p = lambda x, off=0: x.ctypes.data + off   # noqa: E731
        lane.append(lambda nit, a=a, p=p: orbx.lib.orbm_sim3_solve_host(
            p(a["k1"]), p(a["m1"]), n, p(a["t1"]), p(a["k2"]), p(a["m2"]), n, p(a["t2"]), p(w["pts"]), len(w["pts"]),
            p(w["obs_ptr"]), p(a["ob"]), None, p(a["m12"]), C.byref(prm), 0, 0.99, 20, 300, nit, p(a["rd"]),
            p(a["st"]), p(a["st"], 4), p(a["st"], 8), p(a["sim3"]), p(a["i12"]), p(a["a2"]), p(a["st"], 12),
            p(a["st"], 16), p(a["st"], 20), p(a["st"], 24)))
    for nit, key in ((5, "round_nit5"), (300, "find_nit300")):
        t = dev_time(lambda: iterate(nit), args.steps, args.warmup, s)
        out[key + "_ms"] = round(t * 1e3, 4)
        out[key + "_used_mean"] = float(sv.used.float().mean())
        out[key + "_ninliers_mean"] = float(sv.ninliers.float().mean())
        reps = max(1, args.steps // 20)
        t0 = time.perf_counter()
        for _ in range(reps):
            for c in range(nc):
                keep[c]["st"][:2] = 0                          # a new solver each time
                assert lane[c](nit) == orbx.OK
        out[key + "_cpu_lane_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 4)
        out[key + "_cpu_lane_ninliers_mean"] = float(np.mean([a["st"][3] for a in keep]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
