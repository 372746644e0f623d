"""Time of orbm_optimize_sim3_device for a batch, by HIP events (the record in DESIGN.md §5 "Sim3 optimisation").

--pairs KeyFrame pairs (default 8) of --corr correspondences each (default 200): two KeyFrames see the same points
through a Sim3 of scale 1.1, keypoints with 0.5 px of noise, --gross of the correspondences 30 px off, the start 2% /
0.01 rad / 2 cm from the generating Sim3.  d_matches1 is restored before every repetition (the call updates it).
Prints one JSON line: the times of the repetitions in microseconds, and the iterations, rejected trials and nBad of
each pair.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))
import orbx  # noqa: E402

K = (500.0, 500.0, 320.0, 240.0)


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--corr", type=int, default=200)
    ap.add_argument("--gross", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    npairs, n = a.pairs, a.corr
    rng = np.random.default_rng(0)
    scale = np.array([1.2 ** i for i in range(8)], np.float32)
    inv_sigma2 = (1.0 / (scale * scale)).astype(np.float32)
    P = orbx.pose_params(K, (0.0, 640.0, 0.0, 480.0), scale, inv_sigma2=inv_sigma2)
    B = 2 * npairs
    kps = np.zeros((B, n), orbx.KEYPOINT_DTYPE)
    kf_mp = np.full((B, n), -1, np.int32)
    pose = np.zeros((B, 12), np.float32)
    pts = np.zeros(B * n, orbx.MAP_POINT_DTYPE)
    pts["flags"] = 3
    obs = np.zeros(B * n, orbx.OBSERVATION_DTYPE)
    m1 = np.zeros((npairs, n), np.int32)
    sim3 = np.zeros((npairs, 13), np.float32)
    s12 = 1.1
    for p in range(npairs):
        d2 = rng.uniform(4.0, 12.0, n)
        u2, v2 = rng.uniform(60, 580, n), rng.uniform(60, 420, n)
        X2 = np.stack([(u2 - K[2]) / K[0] * d2, (v2 - K[3]) / K[1] * d2, d2], 1)
        R12, t12 = rodrigues(rng.normal(0, 0.08, 3)), rng.normal(0, 0.2, 3)
        X1 = s12 * (X2 @ R12.T) + t12
        for f, X in ((2 * p, X1), (2 * p + 1, X2)):
            T = np.hstack([rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, (3, 1))]).astype(np.float32)
            pose[f] = T.ravel()
            Xw = (X - T[:, 3].astype(np.float64)) @ T[:, :3].astype(np.float64)
            rows = slice(f * n, (f + 1) * n)
            pts["x"][rows], pts["y"][rows], pts["z"][rows] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
            kps["x"][f] = K[0] * X[:, 0] / X[:, 2] + K[2] + rng.normal(0, 0.5, n)
            kps["y"][f] = K[1] * X[:, 1] / X[:, 2] + K[3] + rng.normal(0, 0.5, n)
            kps["octave"][f] = rng.integers(0, 4, n)
            kf_mp[f] = f * n + np.arange(n)
            obs["kf"][rows], obs["idx"][rows] = f, np.arange(n)
        kps["x"][2 * p, :a.gross] += 30.0
        m1[p] = (2 * p + 1) * n + np.arange(n)
        R0 = rodrigues(np.array([0.01, -0.01, 0.005])) @ R12
        sim3[p] = np.concatenate([[s12 * 1.02], R0.ravel(), t12 + 0.02])
    dev = torch.device("cuda", 0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    args = (T(kps.view(np.int32).reshape(B, n, 7)), T(np.full(B, n, np.int32)), T(pose), T(kf_mp),
            T(pts.view(np.int32).reshape(-1, 12)), T(np.arange(B * n + 1, dtype=np.int32)),
            T(obs.view(np.int32).reshape(-1, 2)), T(np.arange(0, B, 2, dtype=np.int32)),
            T(np.arange(1, B, 2, dtype=np.int32)), T(sim3))
    d_m0 = T(m1)
    d_m1 = d_m0.clone()
    out = orbx.optimize_sim3_device(*args, d_m1, P)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        d_m1.copy_(d_m0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orbx.optimize_sim3_device(*args, d_m1, P, sim3_out=out[0], sim3f_out=out[1], scw=out[2], nin=out[3],
                                        trace=out[4], status=out[5])
        e1.record()
        torch.cuda.synchronize()
        times.append(round(e0.elapsed_time(e1) * 1e3, 1))
    tr = out[4].cpu().numpy()
    print(json.dumps(dict(pairs=npairs, corr=n, gross=a.gross, us=times, status=out[5].cpu().tolist(),
                          nin=out[3].cpu().tolist(), iters=tr[:, 0:2].tolist(), rejected=tr[:, 2:4].tolist(),
                          nbad=tr[:, 4].tolist())))


if __name__ == "__main__":
    main()
