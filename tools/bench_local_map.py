#!/usr/bin/env python3
"""Device time of orbm_local_map_device (Tracking::UpdateLocalMap and the first loop of SearchLocalPoints) at a
TUM-like shape, next to the upload it replaces, in one run, from HIP events over back-to-back calls on the launch
stream with the tables resident.

  python tools/bench_local_map.py [--frames 64] [--features 2000] [--keyframes 400] [--points 100000] [--steps 50]

The map is a corridor: KeyFrame f sees MapPoints of a window around f / keyframes of the map, wide enough that a
frame's matched MapPoints vote for about 80 KeyFrames.  A frame stands where a KeyFrame stands and holds a sample of
its MapPoints.  The upload is the host-packed local map the call makes unnecessary: the orbm_map_point and
descriptor arrays of the listed points and d_claimed, pinned host memory to device on the same stream.
Prints one JSON object: per call and per frame times, the mean list lengths, and the bytes the gather must move
(listed points x (48 + 32) B written, local KeyFrames x cap x 4 B read) as the floor to read the time against.
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


def corridor(rng, nkf, cap, nmp, window):
    """kf_mp (nkf, cap): 60% of the features hold a MapPoint of the KeyFrame's window; the observation lists that
    agree with it as CSR (slot order); a chain of parents; the ten nearest KeyFrames as covisibles."""
    centre = (np.arange(nkf) * (nmp / nkf)).astype(np.int64)
    kf_mp = (centre[:, None] + rng.integers(0, window, (nkf, cap))) % nmp
    kf_mp = np.where(rng.random((nkf, cap)) < 0.4, -1, kf_mp).astype(np.int32)
    f, i = np.nonzero(kf_mp >= 0)
    pairs = np.unique(np.stack([kf_mp[f, i].astype(np.int64), f], 1), axis=0)      # sorted by (MapPoint, slot)
    obs_ptr = np.zeros(nmp + 1, np.int32)
    obs_ptr[1:] = np.cumsum(np.bincount(pairs[:, 0], minlength=nmp))
    obs = np.zeros(len(pairs), orbx.OBSERVATION_DTYPE)
    obs["kf"] = pairs[:, 1]
    parent = np.arange(-1, nkf - 1, dtype=np.int32)
    child_ptr = np.minimum(np.arange(nkf + 1), nkf - 1).astype(np.int32)
    child = np.arange(1, nkf, dtype=np.int32)
    off = np.array([1, -1, 2, -2, 3, -3, 4, -4, 5, -5])
    covis = np.arange(nkf)[:, None] + off[None, :]
    covis = np.where((covis < 0) | (covis >= nkf), -1, covis).astype(np.int32)
    return kf_mp, obs_ptr, obs, parent, child_ptr, child, covis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--matched", type=int, default=300)
    ap.add_argument("--kfcap", type=int, default=96)
    ap.add_argument("--pcap", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    rng = np.random.default_rng(0)
    B, n, nkf, nmp, cap = args.frames, args.features, args.keyframes, args.points, args.features
    window = int(nmp / nkf * 40)                                   # a frame's votes reach ~80 KeyFrames
    kf_mp, obs_ptr, obs, parent, child_ptr, child, covis = corridor(rng, nkf, cap, nmp, window)
    pts = rng.integers(1, 2 ** 30, (nmp, 12)).astype(np.int32)
    pts[:, 10] = (rng.random(nmp) < 0.97).astype(np.int32) | 2    # 3% bad MapPoints
    frame_mp = np.full((B, n), -1, np.int32)
    for b in range(B):
        kf = int(rng.integers(40, nkf - 40))
        own = kf_mp[kf][kf_mp[kf] >= 0]
        frame_mp[b, rng.choice(n, args.matched, replace=False)] = rng.choice(own, args.matched, replace=False)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(counts=torch.full((nkf,), cap, dtype=torch.int32, device=dev), kf_mp=T(kf_mp),
             kf_bad=T((rng.random(nkf) < 0.02).astype(np.uint8)), covis=T(covis), child_ptr=T(child_ptr),
             child=T(child), parent=T(parent), pts=T(pts), pdesc=T(rng.integers(0, 256, (nmp, 32), dtype=np.uint8)),
             obs_ptr=T(obs_ptr), obs=T(obs.view(np.int32).reshape(-1, 2)))
    fr = dict(fcounts=torch.full((B,), n, dtype=torch.int32, device=dev), frame_mp=T(frame_mp),
              local_kf=torch.zeros((B, args.kfcap), dtype=torch.int32, device=dev),
              nlocal_kf=torch.zeros((B,), dtype=torch.int32, device=dev),
              ref_kf=torch.zeros((B,), dtype=torch.int32, device=dev))
    work = orbx.local_map_work(nkf, nmp, B, args.kfcap, dev)
    out = orbx.local_map_device(pcap=args.pcap, work=work, stream=s, **t, **fr)

    def call():
        orbx.local_map_device(pcap=args.pcap, work=work, out=out, stream=s, **t, **fr)
    sec = dev_time(call, args.steps, args.warmup, s)
    status = out["status"].cpu().numpy()
    nl, nk = out["nlocal"].cpu().numpy().astype(np.int64), fr["nlocal_kf"].cpu().numpy().astype(np.int64)
    assert int(work.abs().max()) == 0
    written, read = int(nl.sum()) * 80, int(nk.sum()) * cap * 4
    res = {"bench": "local map batch", "frames": B, "features": n, "keyframes": nkf, "points": nmp,
           "matched_per_frame": args.matched, "steps": args.steps, "status_or": int(np.bitwise_or.reduce(status)),
           "local_keyframes_mean": round(float(nk.mean()), 1), "local_points_mean": round(float(nl.mean()), 1),
           "call_ms": round(sec * 1e3, 4), "per_frame_us": round(sec * 1e6 / B, 2),
           "gather_bytes_written": written, "keyframe_bytes_read": read,
           "floor_gbytes_per_s": round((written + read) / sec * 1e-9, 1),
           "work_mbytes": round(work.numel() * 4 / 2 ** 20, 1)}
    # the upload the call replaces: the host-packed points, descriptors and claims of the same lists
    k = int(nl.max())
    hp = torch.empty((B, k, 12), dtype=torch.int32, pin_memory=True)
    hd = torch.empty((B, k, 32), dtype=torch.uint8, pin_memory=True)
    hc = torch.empty((B, n), dtype=torch.uint8, pin_memory=True)
    dp, dd, dc = (torch.empty(h.shape, dtype=h.dtype, device=dev) for h in (hp, hd, hc))

    def upload():
        dp.copy_(hp, non_blocking=True)
        dd.copy_(hd, non_blocking=True)
        dc.copy_(hc, non_blocking=True)
    res["upload_ms"] = round(dev_time(upload, args.steps, args.warmup, s) * 1e3, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
