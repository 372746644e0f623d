"""Time of orbm_pose_optimization_device for a batch, beside the host round trip it replaces.

Frames from orbx_synth.kitti_sequence are extracted on the device (2,000 features), orbx_synth.pose_scene places
MapPoints on their keypoints, and SearchByProjection(KeyFrame) on the device leaves the matches the optimiser reads:
1,024 frames (--distinct different ones, repeated) with about 300 and about 1,500 matches per frame.  The start pose
is the scene's pose moved by a few centimetres.

Run it under the profiler for the kernel's own time (the record in DESIGN.md §5):

    rocprofv3 --kernel-trace --stats -d out -- python tools/diag/pose_opt_time.py

It also prints HIP-event times of the call and of the round trip a host optimiser needs around its own work: the
copy of d_frame_mp and the poses to the host and of the poses and flags back.

--ticks: with ORBX_LIB pointing at a library whose orbx_poseopt.hip was compiled with -DORBX_PO_DIAG_TICKS, lane 0
counts the shader clock of the ordered sweep and of the whole frame, and the script prints the sweep's share.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))
import orbx  # noqa: E402
import orbx_synth  # noqa: E402

K = (718.856, 718.856, 607.19, 185.22)
BF = 386.14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, D = a.frames, a.distinct
    imgs = orbx_synth.kitti_sequence(D, start=3)
    ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, device=0)
    cap = ex.capacity(imgs.shape[1], imgs.shape[2])
    kps = torch.zeros((D, cap, 7), dtype=torch.int32, device=dev)
    desc = torch.zeros((D, cap, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros((D,), dtype=torch.int32, device=dev)
    ex.extract_batch_device(torch.from_numpy(imgs).to(dev), kps, desc, counts)
    ex.sync(torch.cuda.current_stream())
    host = orbx.keypoints_from_device(kps, counts)
    hdesc = desc.cpu().numpy()
    rep = torch.arange(B, device=dev) % D
    sc = [np.float32(1.2) ** i for i in range(8)]
    pp = orbx.pose_params(K, (0.0, 1241.0, 0.0, 376.0), sc, bf=BF, th=10.0, orb_dist=100)
    mt = orbx.ORBmatcher(0.9, True)
    rng = np.random.default_rng(7)
    for nmp in (340, 2600):
        scenes = [orbx_synth.pose_scene(300 + f, host[f], hdesc[f, :len(host[f])], nmp, K, BF) for f in range(D)]
        ur = torch.full((D, cap), -1.0, dtype=torch.float32, device=dev)
        for f, s in enumerate(scenes):
            ur[f, :len(s[3])] = torch.from_numpy(s[3])
        pts = torch.from_numpy(np.stack([s[1] for s in scenes]).view(np.int32).reshape(D, nmp, 12)).to(dev)
        pdesc = torch.from_numpy(np.stack([s[2] for s in scenes])).to(dev)
        pose = torch.from_numpy(np.stack([np.concatenate([s[0].ravel(), s[0].ravel()]) for s in scenes])).to(dev)
        start = pose.clone()
        start[:, [3, 7, 11]] += torch.from_numpy(rng.normal(0, 0.03, (D, 3)).astype(np.float32)).to(dev)
        # the batch: frame b is distinct frame b % D; one MapPoint table for all, frame b's points at b * nmp
        bk, bd, bu, bc = kps[rep].contiguous(), desc[rep].contiguous(), ur[rep].contiguous(), counts[rep].contiguous()
        bpts, bpd, bpose, bstart = pts[rep].contiguous(), pdesc[rep].contiguous(), pose[rep].contiguous(), start[rep].contiguous()
        npts = torch.full((B,), nmp, dtype=torch.int32, device=dev)
        claimed = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
        match, _ = mt.project_search_batch_device(orbx.PROJ_KEYFRAME, bk, bd, bu, claimed, bc, bpose, bpts, bpd, npts, pp)
        base = (torch.arange(B, device=dev, dtype=torch.int32) * nmp).reshape(B, 1)
        fmp0 = torch.where(match >= 0, match + base, torch.full_like(match, -1)).contiguous()
        table = bpts.reshape(B * nmp, 12)
        outl = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
        res, times = None, []
        for r in range(a.reps + 1):
            fmp = fmp0.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = orbx.pose_optimization_device(bk, bu, bc, fmp, table, bstart, pp, orbx.POSE_OPT_DISCARD, outlier=outl)
            e1.record()
            torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1))
        tr = res[5].cpu().numpy().view(orbx.POSE_OPT_TRACE_DTYPE).reshape(B)
        assert not res[6].any().item()
        # passes: one per round with a level-0 edge, one per Levenberg trial; a trial is either rejected or the one
        # accepted trial that ends an iteration, so trials <= rejected + iters (equal unless an iteration ends
        # without an acceptance, on qmax == 10 or rho == 0)
        passes = (tr["iters"] > 0).sum(1) + tr["rejected"].sum(1) + tr["iters"].sum(1)
        msg = ("matches/frame %.0f (features %.0f): call %.3f ms per batch by events (best of %d), %.2f us per frame; "
               "inliers %.0f, rounds %.1f, passes per frame <= %.1f"
               % (tr["ncorr"].mean(), bc.float().mean().item(), min(times), a.reps, 1e3 * min(times) / B,
                  res[3].float().mean().item(), tr["rounds"].mean(), passes.mean()))
        if a.ticks:
            sw, fr = tr["nbad"][:, 2].astype(np.float64), tr["nbad"][:, 3].astype(np.float64)
            msg += "; ordered sweep %.1f%% of the frame's clock (lane 0: %.0f of %.0f ticks)" % (
                100 * sw.sum() / fr.sum(), sw.mean(), fr.mean())
        print(msg, flush=True)
        # the round trip of a host optimiser: matches and poses down, poses and flags up
        h_mp = torch.empty((B, cap), dtype=torch.int32).pin_memory()
        h_pose = torch.empty((B, 24), dtype=torch.float32).pin_memory()
        h_out = torch.zeros((B, cap), dtype=torch.uint8).pin_memory()
        rt = []
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h_mp.copy_(fmp0, non_blocking=True)
            h_pose.copy_(bstart, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            bstart.copy_(h_pose, non_blocking=True)
            outl.copy_(h_out, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            if r:
                rt.append(e0.elapsed_time(e1))
        print("    host round trip of the copies alone: %.3f ms per batch" % min(rt), flush=True)


if __name__ == "__main__":
    main()
