#!/usr/bin/env python3
"""Device time of LocalMapping's culls over the resident KeyFrame and MapPoint tables, from HIP events over
back-to-back calls on the launch stream with the inputs resident, at a SLAM-sized map: 200 KeyFrames of about 2,000
features, MapPoints with 8 observations each.

  keyframes   orbm_keyframe_culling_device: 60 candidates, 6 of them (10 %) culled
  mappoints   orbm_map_point_culling_device: a recent list of 2,000 MapPoints, about 10 % culled
  compaction  orbm_compact_observations_device over the whole observation CSR after both

  python tools/bench_culling.py [--steps 200] [--runs 2]

A cull edits the tables, so each timed step first puts them back (device-to-device copies of d_kf_mp, the flags,
the mask, d_ref and d_nobs); that restore is timed alone as well and taken off.  transfer_ms is what the host pass
these calls replace pays before it starts: d_kf_mp and the observation CSR over the link, once each way, at the 57
GB/s the project measured (docs/EXPERIMENTS.md).  The split into kernels comes from a kernel trace, in a run of its
own (tracing slows the host):

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_culling.py --steps 10 --runs 1

Prints one JSON object per case and run.
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

LINK_GBS = 57.0
NLEVELS = 8


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


def build(nkf, nfeat, nobs, ncand, nculled, seed=0):
    """KeyFrames along a track: MapPoint m is seen by nobs of the 2 * nobs KeyFrames that follow its first one, so
    every KeyFrame holds about nfeat MapPoints.  The candidates of KeyFrame 0 are the ncand KeyFrames behind it.
    Features sit on random levels, which leaves about four in five MapPoints of a KeyFrame redundant; nculled
    candidates, spread over the list, have all theirs on the coarsest level, where every other observation is fine
    enough."""
    rng = np.random.default_rng(seed)
    per = nfeat // nobs
    nmp = nkf * per
    first = np.repeat(np.arange(nkf), per)
    offs = np.argsort(rng.random((nmp, 2 * nobs)), 1)[:, :nobs]
    seen = np.sort((first[:, None] + offs) % nkf, 1)               # the observers of every MapPoint, ascending
    flat = seen.reshape(-1)
    order = np.argsort(flat, kind="stable")
    counts = np.bincount(flat, minlength=nkf).astype(np.int32)
    cap = int(counts.max())
    start = np.concatenate([[0], np.cumsum(counts)])
    idx = np.empty(nmp * nobs, np.int32)                           # the feature index of every observation
    idx[order] = np.arange(nmp * nobs) - start[flat[order]]
    obs = np.zeros(nmp * nobs, orbx.OBSERVATION_DTYPE)
    obs["kf"], obs["idx"] = flat, idx
    kf_mp = np.full((nkf, cap), -1, np.int32)
    kf_mp[flat, idx] = np.repeat(np.arange(nmp), nobs)
    pts = np.zeros(nmp, orbx.MAP_POINT_DTYPE)
    pts["flags"] = 3
    cands = np.arange(1, ncand + 1, dtype=np.int32)
    kps = np.zeros((nkf, cap), orbx.KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, NLEVELS, (nkf, cap))
    kps["octave"][cands[::max(ncand // max(nculled, 1), 1)][:nculled]] = NLEVELS - 1
    ref = obs[::nobs].copy()
    return dict(nkf=nkf, nmp=nmp, cap=cap, counts=counts, kf_mp=kf_mp, obs=obs, kps=kps, pts=pts, ref=ref,
                obs_ptr=(np.arange(nmp + 1) * nobs).astype(np.int32), nobs=np.full(nmp, nobs, np.int32), cands=cands)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=60)
    ap.add_argument("--culled", type=int, default=6)
    ap.add_argument("--recent", type=int, default=2000)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nobs_per, ccap = 8, 64
    w = build(args.keyframes, args.features, nobs_per, args.candidates, args.culled)
    nkf, nmp, cap = w["nkf"], w["nmp"], w["cap"]
    rng = np.random.default_rng(1)
    counts, kf_mp, obs_ptr = T(w["counts"]), T(w["kf_mp"]), T(w["obs_ptr"])
    obs, pts = T(w["obs"].view(np.int32).reshape(-1, 2)), T(w["pts"].view(np.int32).reshape(-1, 12))
    kps = T(w["kps"].view(np.int32).reshape(nkf, cap, 7))
    ref, nobs = T(w["ref"].view(np.int32).reshape(-1, 2)), T(w["nobs"])
    erased = torch.zeros(len(w["obs"]), dtype=torch.uint8, device=dev)
    noterase = torch.zeros(nkf, dtype=torch.uint8, device=dev)
    g = orbx.covis_graph(nkf, ccap, dev)
    g["ord_kf"][0, :args.candidates] = T(w["cands"])
    g["nord"][0] = args.candidates
    work = orbx.culling_work(nmp, dev)
    recent = T(rng.permutation(nmp)[:args.recent].astype(np.int32))
    visible = torch.full((nmp,), 100, dtype=torch.int32, device=dev)
    found = T(np.where(rng.random(nmp) < 0.1, 20, 60).astype(np.int32))      # about 10 % below a quarter
    first = torch.full((nmp,), 99, dtype=torch.int32, device=dev)
    state = dict(kf_mp=kf_mp, pts=pts, erased=erased, ref=ref, nobs=nobs)
    state0 = {k: v.clone() for k, v in state.items()}
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    ko = dict(verdict=i32(ccap), nmps=i32(ccap), nred=i32(ccap), culled=i32(ccap), nculled=i32(1), ncand=i32(1))
    mo = dict(verdict=i32(args.recent), recent_out=i32(args.recent), nrecent_out=i32(1))
    co = dict(obs_ptr=i32(nmp + 1), obs=torch.zeros_like(obs), status=i32(1))

    def restore():
        for k in state:
            state[k].copy_(state0[k])

    def keyframes():
        orbx.keyframe_culling_device(g, 0, counts, kf_mp, kps, None, 35.0, False, NLEVELS, noterase, pts, obs_ptr, obs,
                                     erased, ref, nobs, work, root=-1, out=ko, stream=s)

    def mappoints():
        orbx.map_point_culling_device(recent, 100, 2, counts, kf_mp, pts, obs_ptr, obs, erased, nobs, found, visible,
                                      first, out=mo, stream=s)

    def compaction():
        orbx.compact_observations_device(obs_ptr, obs, erased, out=co, stream=s)

    table_bytes = kf_mp.numel() * 4 + obs_ptr.numel() * 4 + obs.numel() * 4
    transfer_ms = 2 * table_bytes / (LINK_GBS * 1e9) * 1e3
    for run in range(args.runs):
        t_restore = dev_time(restore, args.steps, args.warmup, s)
        t_kf = dev_time(lambda: (restore(), keyframes()), args.steps, args.warmup, s)
        nculled = int(ko["nculled"][0])
        verdict = ko["verdict"][:args.candidates].cpu().numpy()
        assert int(ko["ncand"][0]) == args.candidates and (verdict != orbx.KFCULL_INVALID).all()
        assert int(work.count_nonzero()) == 0
        t_mp = dev_time(lambda: (restore(), mappoints()), args.steps, args.warmup, s)
        mv = mo["verdict"].cpu().numpy()
        assert (mv != orbx.CULL_INVALID).all()
        restore()
        mappoints()
        keyframes()
        t_co = dev_time(compaction, args.steps, args.warmup, s)
        assert int(co["status"][0]) == 0
        common = dict(bench="culling", run=run, keyframes=nkf, features=int(w["counts"].mean()), map_points=nmp,
                      obs_per_point=nobs_per, steps=args.steps, restore_ms=round(t_restore * 1e3, 4),
                      table_mbytes=round(table_bytes / 1e6, 2), transfer_ms=round(transfer_ms, 4))
        print(json.dumps(dict(common, case="keyframes", candidates=args.candidates, culled=nculled,
                              call_ms=round((t_kf - t_restore) * 1e3, 4),
                              per_candidate_us=round((t_kf - t_restore) * 1e6 / args.candidates, 2))), flush=True)
        print(json.dumps(dict(common, case="mappoints", recent=args.recent,
                              culled=int(((mv == orbx.CULL_RATIO) | (mv == orbx.CULL_OBS)).sum()),
                              kept=int(mo["nrecent_out"][0]), call_ms=round((t_mp - t_restore) * 1e3, 4))), flush=True)
        print(json.dumps(dict(common, case="compaction", live=int(co["obs_ptr"][-1]), entries=int(obs.shape[0]),
                              call_ms=round(t_co * 1e3, 4))), flush=True)


if __name__ == "__main__":
    main()
