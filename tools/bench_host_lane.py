#!/usr/bin/env python3
"""Wall time of the synchronous host entry points (staging through HostCall, the device call, the copies back and
the stream synchronisation), per call, on the tables of tools/bench_culling.py and tools/bench_triangulate.py at a
size where the staging is a visible share of the call:

  map_point_culling     orbm_map_point_culling, a recent list of 200 MapPoints over 20 KeyFrames of about 200 features
  compact_observations  orbm_compact_observations over that table's observation CSR
  triangulate           orbm_triangulate, one pair of 300 matches
  stereo_band           orbm_stereo_band, 3,000 left and 2,500 right keypoints
  allpairs_top2         orbm_allpairs, 2,000 x 2,000 descriptors

  python tools/bench_host_lane.py [--steps 2000]

Prints one JSON object: the median, the mean and the 10th percentile of every call in microseconds.  To compare two
builds, alternate them (ORBX_LIB names the library to load) and look at the spread of one build's repeated runs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "orb-slam-_amd"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402

import orbx  # noqa: E402
import orbx_synth  # noqa: E402
from bench_culling import build as culling_tables  # noqa: E402
from bench_triangulate import BF, BOUNDS, K, SCALE, build as triangulate_tables  # noqa: E402


def wall_time(call, steps, warmup):
    for _ in range(warmup):
        call()
    t = np.empty(steps)
    for i in range(steps):
        t0 = time.perf_counter()
        call()
        t[i] = (time.perf_counter() - t0) * 1e6
    return dict(median_us=round(float(np.median(t)), 2), mean_us=round(float(t.mean()), 2),
                p10_us=round(float(np.percentile(t, 10)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    out = {"bench": "host_lane", "steps": args.steps}
    time_it = lambda call: wall_time(call, args.steps, args.warmup)

    w = culling_tables(20, 200, 8, 6, 1)
    nmp = w["nmp"]
    recent = rng.permutation(nmp)[:200].astype(np.int32)
    found = np.where(rng.random(nmp) < 0.1, 20, 60).astype(np.int32)
    visible, first = np.full(nmp, 100, np.int32), np.full(nmp, 99, np.int32)
    erased = np.zeros(len(w["obs"]), np.uint8)
    # the cull edits its tables: every call gets the same ones again (the copies are part of the timed call, and
    # the same for every build)
    out["map_point_culling"] = time_it(lambda: orbx.map_point_culling(
        recent, 100, 2, w["counts"], w["kf_mp"].copy(), w["pts"].copy(), w["obs_ptr"], w["obs"], erased.copy(),
        w["nobs"], found, visible, first))
    out["compact_observations"] = time_it(lambda: orbx.compact_observations(w["obs_ptr"], w["obs"], erased))

    t = triangulate_tables(1, 300, 0.3)
    pp = orbx.pose_params(K, BOUNDS, SCALE, bf=BF)
    out["triangulate"] = time_it(lambda: orbx.triangulate(
        t["kps"][0], t["pose"][0], t["kps"][1], t["pose"][1], t["match"][0], pp, uright1=t["uright"][0],
        depth1=t["depth"][0], uright2=t["uright"][1], depth2=t["depth"][1]))

    def side(n):
        k = np.zeros(n, orbx.KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"] = rng.uniform(0, 752, n), rng.uniform(0, 480, n), rng.integers(0, 8, n)
        return k, orbx_synth.random_descriptors(n, n)
    (kl, dl), (kr, dr) = side(3000), side(2500)
    out["stereo_band"] = time_it(lambda: orbx.stereo_band(kl, dl, kr, dr, 480, SCALE, 0.0, 110.0))
    q, d = orbx_synth.random_descriptors(2000, 1), orbx_synth.random_descriptors(2000, 2)
    out["allpairs_top2"] = time_it(lambda: orbx.allpairs_host(q, d))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
