#!/usr/bin/env python3
"""Device time of the batched Initializer (Tracking::MonocularInitialization's Initialize after
SearchForInitialization) beside the same work in the CPU lane (orbm_initialize_host, the kernels' code on one core),
in one run.

  python tools/bench_initializer.py [--pairs 1,64,4096] [--matches 300] [--iterations 200] [--runs 2]

Reports, from HIP events over back-to-back calls on the launch stream after warm-up, with the inputs resident: the
time of one orbm_initialize_device call (its five launches included) for every batch size, `runs` times, and the time
of orbm_initialize_host per pair over a sample of the same pairs.  The number of timed calls adapts to the call's
length (about a second per figure).
The scenes are synthetic: 16 two-view scenes (every other one a plane) of `matches` matches, a tenth of them wrong,
half a pixel of noise; a batch tiles them over its pairs, each pair with draws of its own.
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
NSCENES = 16


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def scene(seed, n, plane):
    """(kps1, kps2, matches12): n matched keys and a few unmatched ones per frame."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(30, BOUNDS[1] - 30, n), rng.uniform(30, BOUNDS[3] - 30, n)
    d = 12.0 + 0.004 * (u - K[2]) if plane else rng.uniform(6.0, 30.0, n)
    X = np.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], 1)
    R, t = rodrigues(rng.normal(0, 0.03, 3)), np.array([0.8, 0.05, 0.1]) + rng.normal(0, 0.05, 3)
    Y = X @ R.T + t
    xy1 = np.stack([u, v], 1) + rng.normal(0, 0.5, (n, 2))
    xy2 = np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], 1) + rng.normal(0, 0.5, (n, 2))
    extra = n // 15
    k1 = np.zeros(n + extra, orbx.KEYPOINT_DTYPE)
    k2 = np.zeros(n + extra, orbx.KEYPOINT_DTYPE)
    perm = rng.permutation(n)
    k1["x"][:n], k1["y"][:n] = xy1.T
    k2["x"][perm], k2["y"][perm] = xy2.T
    for k in (k1, k2):
        k["x"][n:], k["y"][n:] = rng.uniform(0, BOUNDS[1], extra), rng.uniform(0, BOUNDS[3], extra)
    m12 = np.full(n + extra, -1, np.int32)
    m12[:n] = perm
    wrong = n // 10
    m12[:wrong] = np.roll(m12[:wrong], 1)
    return k1, k2, m12


def dev_time(fn, stream, budget=1.0):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    steps = int(min(2000, max(2, budget / max(time.perf_counter() - t0, 1e-5))))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e-3, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,4096")
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    it = args.iterations
    scenes = [scene(100 + q, args.matches, q % 2 == 1) for q in range(NSCENES)]
    cap = len(scenes[0][0])
    P = orbx.pose_params(K, BOUNDS, SCALE)
    prm = orbx.PoseParams.from_buffer_copy(P)
    kps = np.zeros((2 * NSCENES, cap), orbx.KEYPOINT_DTYPE)
    for q, (k1, k2, _) in enumerate(scenes):
        kps[2 * q], kps[2 * q + 1] = k1, k2
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_kps, d_counts = T(kps.view(np.int32).reshape(2 * NSCENES, cap, 7)), T(np.full(2 * NSCENES, cap, np.int32))
    out = {"bench": "Initializer batch", "matches": args.matches, "cap": cap, "iterations": it, "runs": []}
    for run in range(args.runs):
        res = {}
        for npairs in (int(x) for x in args.pairs.split(",")):
            rng = np.random.default_rng(npairs + run)
            q = np.arange(npairs) % NSCENES
            draws = rng.integers(0, 2 ** 31, (npairs, 8 * it)).astype(np.int32)
            m12 = np.stack([scenes[i][2] for i in q])
            ini = orbx.Initializer(npairs, cap, P, dev, max_iterations=it)
            tabs = (d_kps, d_counts, T((2 * q).astype(np.int32)), T((2 * q + 1).astype(np.int32)), T(m12), T(draws))
            t, steps = dev_time(lambda: ini.initialize(*tabs, prune_matches=True, stream=s), s)
            st = ini.status.cpu().numpy()[:, 0]
            res[str(npairs)] = {"call_ms": round(t * 1e3, 4), "steps": steps, "ok": int((st == 0).sum()),
                                "failed": int((st == 4).sum()), "model_H": int((ini.model == 1).sum().item()),
                                "workspace_MB": round(ini.work_bytes / 2 ** 20, 1)}
            # the CPU lane on a sample of the same pairs: argument lists built once, the timed loop is the C calls
            sample = min(npairs, NSCENES)
            arr = {f: np.zeros(max(sz if isinstance(sz, int) else 3 * cap, 1), dt) for f, dt, sz in orbx._INIT_FIELDS}
            o = orbx.InitOut(**{f: a.ctypes.data for f, a in arr.items()})
            calls = []
            for p in range(sample):
                k1, k2, m = scenes[q[p]]
                calls.append((k1.ctypes.data, cap, k2.ctypes.data, cap, m.ctypes.data, draws[p].ctypes.data,
                              C.byref(prm), 1.0, it, orbx.INIT_PRUNE_MATCHES, C.byref(o)))
            t0 = time.perf_counter()
            for a in calls:
                assert orbx.lib.orbm_initialize_host(*a) == orbx.OK
            res[str(npairs)]["cpu_lane_ms_per_pair"] = round((time.perf_counter() - t0) / sample * 1e3, 4)
            del ini
        out["runs"].append(res)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
