#!/usr/bin/env python3
"""Device time per call of the projection matchers' batched entry points -- orbm_search_by_projection_device,
orbm_project_search_device in its five modes, orbm_search_by_sim3_device -- from HIP events over back-to-back
calls on one stream with the inputs resident.

  python tools/bench_proj.py [--lib liborbx.so ...] [--rounds 9] [--steps 300]

With several --lib (builds of the same ABI, e.g. the parent commit's twice and this tree's) every round times
each of them in turn in this one process, so their numbers share the clock and the neighbours; the outputs of
all builds must be identical.  Per entry point and build: the median and the minimum over the rounds.
Local-map and pose searches: 20 frames x 1000 features x 1500 MapPoints from the test suite's scene()
generators; SearchBySim3: tools/bench_sim3.py's scene (32 candidates x 2000 features).  Prints one JSON object.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("orb-slam-_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_sim3  # noqa: E402
import orbx  # noqa: E402
import test_pose_search as tps  # noqa: E402
import test_proj as tpj  # noqa: E402

FRAMES, FEATURES, POINTS = 20, 1000, 1500


def stack(rows, dtype, words):
    a = np.zeros((len(rows), len(rows[0])) + rows[0].shape[1:], dtype)
    for b, r in enumerate(rows):
        a[b] = r
    return np.ascontiguousarray(a).view(np.int32).reshape(len(rows), len(rows[0]), words) if words else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", help="a liborbx.so to time (repeatable); default: this tree's")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    paths = args.lib or [orbx.LIB_PATH]
    libs = [C.CDLL(os.path.abspath(p)) for p in paths]
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(s.cuda_stream)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    keep, entries = [], {}   # entries: name -> (call(lib), outputs)

    # local-map search
    sc = [tpj.scene(f, n_kp=FEATURES, n_mp=POINTS) for f in range(FRAMES)]
    a = [T(stack([x[0] for x in sc], orbx.KEYPOINT_DTYPE, 7)), T(stack([x[1] for x in sc], np.uint8, 0)),
         T(stack([x[2] for x in sc], np.float32, 0)), T(stack([x[3] for x in sc], np.uint8, 0)),
         torch.full((FRAMES,), FEATURES, dtype=torch.int32, device=dev),
         T(stack([x[5] for x in sc], orbx.PROJ_POINT_DTYPE, 6)), T(stack([x[6] for x in sc], np.uint8, 0)),
         torch.full((FRAMES,), POINTS, dtype=torch.int32, device=dev)]
    prm = orbx.proj_params(sc[0][4], tpj.SCALE, 3.0, 0.8)
    m, n = i32(FRAMES, FEATURES), i32(FRAMES)
    keep += [a, prm]
    entries["search_by_projection"] = (
        lambda L, a=a, prm=prm, m=m, n=n: L.orbm_search_by_projection_device(
            P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), FRAMES, FEATURES, P(a[5]), P(a[6]), P(a[7]), POINTS,
            C.byref(prm), P(m), P(n), st), (m, n))

    # pose searches
    for mode in tps.MODES:
        sim3 = mode in ("sim3", "fuse_sim3")
        sc = [tps.scene(f, n_kp=FEATURES, n_mp=POINTS, sim3_scale=1.7 if sim3 else 1.0) for f in range(FRAMES)]
        pose = np.stack([np.concatenate([x[5].ravel(), np.zeros(12, np.float32)]) if sim3 else x[4] for x in sc])
        a = [T(stack([x[0] for x in sc], orbx.KEYPOINT_DTYPE, 7)), T(stack([x[1] for x in sc], np.uint8, 0)),
             T(stack([x[2] for x in sc], np.float32, 0)), T(stack([x[3] for x in sc], np.uint8, 0)),
             torch.full((FRAMES,), FEATURES, dtype=torch.int32, device=dev), T(pose.astype(np.float32)),
             T(stack([x[6] for x in sc], orbx.MAP_POINT_DTYPE, 12)), T(stack([x[7] for x in sc], np.uint8, 0)),
             torch.full((FRAMES,), POINTS, dtype=torch.int32, device=dev)]
        prm = orbx.PoseParams.from_buffer_copy(tps.params(**tps.CASES[mode][0]))
        m, n = i32(FRAMES, FEATURES if tps.MODE_ID[mode] <= 2 else POINTS), i32(FRAMES)
        keep += [a, prm]
        entries["project_search_" + mode] = (
            lambda L, a=a, prm=prm, m=m, n=n, mode=mode: L.orbm_project_search_device(
                tps.MODE_ID[mode], P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), FRAMES, FEATURES, P(a[5]), P(a[6]),
                P(a[7]), P(a[8]), POINTS, C.byref(prm), P(m), P(n), st), (m, n))

    # SearchBySim3
    nc, nf = 32, 2000
    w = bench_sim3.build(nc, nf, 1.7)
    rng = np.random.default_rng(1)
    a = [T(w["kps"].view(np.int32).reshape(nc + 1, nf, 7)), T(w["desc"]),
         T(w["mps"].view(np.int32).reshape(nc + 1, nf, 12)), T(w["mpdesc"]),
         torch.full((nc + 1,), nf, dtype=torch.int32, device=dev), T(w["pose"]),
         torch.zeros((nc,), dtype=torch.int32, device=dev), torch.arange(1, nc + 1, dtype=torch.int32, device=dev),
         T(w["sim3"]), T((rng.random((nc, nf)) < 0.1).astype(np.uint8)), T((rng.random((nc, nf)) < 0.1).astype(np.uint8))]
    prm = orbx.pose_params(bench_sim3.K, bench_sim3.BOUNDS, bench_sim3.SCALE, th=7.5)
    m, n = i32(nc, nf), i32(nc)
    keep += [a, prm]
    entries["search_by_sim3"] = (
        lambda L, a=a, prm=prm, m=m, n=n: L.orbm_search_by_sim3_device(
            P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), nc + 1, nf, P(a[5]), P(a[6]), P(a[7]), P(a[8]), P(a[9]),
            P(a[10]), nc, C.byref(prm), P(m), P(n), None, None, st), (m, n))

    out = {"bench": "projection matchers", "libs": paths, "frames": FRAMES, "features": FEATURES, "points": POINTS,
           "sim3_pairs": nc, "sim3_features": nf, "rounds": args.rounds, "steps": args.steps, "ms": {}}
    for name, (call, outs) in entries.items():
        ref = None
        for L in libs:   # warm-up, and the builds' outputs side by side
            for _ in range(args.warmup):
                assert call(L) == 0, name
            torch.cuda.synchronize()
            got = [o.cpu().numpy().copy() for o in outs]
            ref = ref or got
            assert all(np.array_equal(x, y) for x, y in zip(ref, got)), "%s: builds disagree" % name
        out.setdefault("nmatches_mean", {})[name] = float(ref[1].mean())
        ms = [[] for _ in libs]
        for _ in range(args.rounds):
            for k, L in enumerate(libs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(args.steps):
                    call(L)
                e1.record(s)
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.steps)
        out["ms"][name] = [{"median": round(statistics.median(x), 4), "min": round(min(x), 4)} for x in ms]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
