#!/usr/bin/env python3
"""Headline benchmark: BASELINE.json config 2 (KITTI 1241x376 grayscale, 2000
features, 8 levels, scale 1.2) ORB extract + match on MI355X, weak-scaled over
1..N GPUs (config 4: frames sharded per rank, keypoints/descriptors gathered to
rank 0 over RCCL).

One step = per rank, one batch of `--batch` consecutive frames of the synthetic
KITTI replay (already resident in HBM):
  ORBextractor::operator() on every frame     (orbx_extract_batch_device)
  SearchForInitialization(t-1, t) r=100        (orbm_search_init_batch_device,
                                                ORBmatcher(0.9, true) like
                                                Tracking::MonocularInitialization)
  gather of the padded keypoints/descriptors to rank 0 (N > 1)

A plain run sets up, warms up, times `--steps` steps and prints ONE JSON line on rank 0 (`value`, `ms_per_step`,
the configuration, keypoints and matches per frame).  `--dump-outputs DIR` also writes what the last timed step
computed as DIR/<name>.npy.  `--full` adds, after the timed region and outside `value`, everything else the
line can carry: the per-stage breakdown from an instrumented second pass, the isolated one-stream pass and the
rooflines, the achievable-bandwidth probe, the rank-0 ingress proxy, the host-fed leg and the CPU baselines.

Launch:
  python bench.py [--steps K --warmup W] [--full]              (1 GPU)
  python bench.py --gpus N [...]                               (N GPUs: starts the ranks itself)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N
Without a launcher (WORLD_SIZE unset), `--gpus N` > 1 starts
`python -m torch.distributed.run --nproc-per-node N bench.py <same args>` as a
child process before anything touches the GPU, relays rank 0's JSON line and
exits with the child's status (`--dry-run` prints that command instead).  Under
a launcher, `--gpus` must equal WORLD_SIZE.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-_amd"))

DEFAULT_BATCH = 4096   # frames per GPU per step (tools/pmc_summary.py and tools/sq_summary.py read it from here)


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_plan(argv, env):
    """Decide how this invocation runs, before any GPU call.

    Returns ("run", world) to run in this process, ("error", message) for a --gpus / WORLD_SIZE mismatch,
    or ("spawn", cmd) with the torch.distributed.run command that starts `--gpus` ranks of this script
    with the same arguments (rendezvous on 127.0.0.1)."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--dry-run", action="store_true")
    a, _ = ap.parse_known_args(argv)
    if "WORLD_SIZE" in env:   # under torchrun (the driver's N > 1 form, or our own child)
        world = int(env["WORLD_SIZE"])
        if a.gpus is not None and a.gpus != world:
            return "error", "bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world)
        return "run", world
    n = 1 if a.gpus is None else a.gpus
    if n < 1:
        return "error", "bench.py: --gpus must be >= 1"
    if n == 1:
        return "run", 1
    child_args = [x for x in argv if x != "--dry-run"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr=127.0.0.1", "--master-port=%d" % _free_port(), os.path.abspath(__file__)] + child_args
    return "spawn", cmd


def visible_gpu_count(env, kfd_nodes="/sys/class/kfd/kfd/topology/nodes"):
    """GPUs this process could use, counted without any HIP call: the KFD topology nodes with a GPU target
    (gfx_target_version != 0; CPU nodes have 0), narrowed by the *_VISIBLE_DEVICES lists the ROCm runtime
    honours.  None when neither is readable (the caller then lets the ranks find out)."""
    n = None
    try:
        n = 0
        for d in os.listdir(kfd_nodes):
            try:
                with open(os.path.join(kfd_nodes, d, "properties")) as f:
                    props = dict(l.split(None, 1) for l in f if len(l.split(None, 1)) == 2)
                if int(props.get("gfx_target_version", "0")) != 0:
                    n += 1
            except (OSError, ValueError):
                continue
    except OSError:
        n = None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v is not None:
            k = len([x for x in v.split(",") if x.strip() != ""])
            n = k if n is None else min(n, k)
    return n


def spawn_ranks(cmd) -> int:
    """Run the torchrun child, relay rank 0's JSON line to stdout (everything else to stderr, line by line,
    so a long run keeps showing progress) and return the child's exit status.  A child process, never an
    exec: this process has not touched the GPU and never will."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL over dmabuf IPC (the host driver's only mode)
    env["PYTHONUNBUFFERED"] = "1"
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, text=True, env=env)
    for line in p.stdout:
        s = line.strip()
        if s.startswith("{") and '"metric"' in s:
            print(s, flush=True)
        else:
            sys.stderr.write(line)
            sys.stderr.flush()
    return p.wait()


if __name__ == "__main__":
    _mode, _what = launch_plan(sys.argv[1:], os.environ)
    if _mode == "error":
        print(_what, file=sys.stderr, flush=True)
        sys.exit(2)
    if _mode == "spawn":
        if "--dry-run" in sys.argv[1:]:
            print(json.dumps({"launch": _what}), flush=True)
            sys.exit(0)
        _n = next(int(x.split("=")[1]) for x in _what if x.startswith("--nproc-per-node="))
        _vis = visible_gpu_count(os.environ)   # sysfs and env only: this process never initialises HIP
        if _vis is not None and _vis < _n:
            print("bench.py: --gpus %d but %d GPU(s) visible" % (_n, _vis), file=sys.stderr)
            sys.exit(2)
        sys.exit(spawn_ranks(_what))
    if "--dry-run" in sys.argv[1:]:
        print(json.dumps({"launch": None, "world_size": _what}), flush=True)
        sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import orbx  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from srchash import kernel_sources_sha256  # noqa: E402
import orbx_dist  # noqa: E402
import orbx_synth  # noqa: E402

BASELINE = json.load(open(os.path.join(ROOT, "BASELINE.json")))
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# VALU issue peaks measured on the MI355X by tools/probes/valu_rate.hip (profiles/r02/valu_rate.json): the
# kernels' dominant instructions (v_pk_maximum3_f16 in FAST, v_dot4_u32_u8 / v_alignbyte_b32 in describe and the
# pyramid, v_perm_b32) issue once per 4 cycles per SIMD (about 545-580 G wave-instr/s over the chip at 8 waves
# per SIMD), plain ALU ops (v_xor_b32, v_fma_f32) once per 2 (about 990-1050).  A kernel's VALU fraction is taken
# against the measured rate of its dominant instruction.
VALU_RATES = os.path.join(ROOT, "profiles", "r02", "valu_rate.json")
VALU_DOMINANT = {"k_fast_cells": "v_pk_maximum3_f16", "k_describe": "v_dot4_u32_u8", "k_pyramid_level": "v_dot4_u32_u8",
                 "k_quadtree<512,16|512,8|256,4>": "v_xor_b32", "k_si_grid+k_si_build+k_si_greedy": "v_bcnt_u32_b32"}


def valu_peak(kname):
    """(peak G wave-instr/s of the kernel's dominant instruction at 8 waves/SIMD, instruction, 2-cycle class peak)."""
    try:
        d = json.load(open(VALU_RATES))
        ins = VALU_DOMINANT.get(kname, "v_pk_maximum3_f16")
        return float(d["rates"][ins][-1]), ins, float(d["rates"]["v_xor_b32"][-1])
    except Exception:
        return 614.4, "assumed 4 cycles per wave64 instruction", 1228.8
W, H, NFEAT, NLEVELS, SCALE, INI, MINTH = 1241, 376, 2000, 8, 1.2, 20, 7
WINDOW, NNRATIO = 100, 0.9


def copy_bandwidth(dev, nbytes: int = 1 << 30, reps: int = 10):
    """Achievable HBM bandwidth on this GPU, the practical ceiling beside the 8 TB/s spec peak:
    the best of a 16-byte-per-lane streaming copy kernel (tools/probes/hbm_copy.hip; launch shapes, loads per
    lane and non-temporal hints swept, best of 3 groups of 10 copies each) over a 1 GiB buffer, read + write
    bytes per second.  The torch
    device-to-device copy of the same buffers is reported beside it."""
    import ctypes
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    a.fill_(1)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, groups=1):
        fn()
        torch.cuda.synchronize()
        best = 0.0
        for _ in range(groups):
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = max(best, 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        return best

    out = {"torch_copy_GBps": round(timed(lambda: b.copy_(a)), 1)}
    lib_path = os.path.join(ROOT, "tools", "probes", "libhbm_copy.so")
    best, cfg = 0.0, None
    if os.path.exists(lib_path):
        lib = ctypes.CDLL(lib_path)
        lib.hbm_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_void_p]
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        # blocks 0 = one workgroup per contiguous 256 x unroll chunk (the fastest shape on MI355X, 6.5 TB/s),
        # otherwise a grid-stride loop over that many workgroups
        for blocks in (0, 1024, 4096):
            for unroll in (1, 2, 4):
                for nt in (0, 1):
                    def run():
                        if lib.hbm_copy(b.data_ptr(), a.data_ptr(), nbytes // 16, blocks, unroll, nt, st) != 0:
                            raise RuntimeError("hbm_copy launch failed")
                    g = timed(run, groups=3)
                    if g > best:
                        best, cfg = g, {"blocks": blocks or "n/(256*unroll)", "threads": 256,
                                        "uint4_per_thread" if blocks == 0 else "uint4_per_trip": unroll,
                                        "nontemporal": nt}
    del a, b
    out.update({"kernel_copy_GBps": round(best, 1), "kernel_copy_config": cfg})
    return (best if best > 0 else out["torch_copy_GBps"]), out


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def level_sizes():
    inv = [np.float32(1.0)]
    s = np.float32(1.0)
    for _ in range(1, NLEVELS):
        s = np.float32(np.float64(s) * np.float64(np.float32(SCALE)))
        inv.append(np.float32(1.0) / s)
    return [(int(np.rint(np.float32(W) * i)), int(np.rint(np.float32(H) * i))) for i in inv]


_NATIVE = {"built": None}


def native_oracle():
    """Build the CPU-baseline copy of oracle/orbref.c on this host with -march=native (the reference's own
    flag) and point orbref at it (ORBREF_LIB).  Parity tests keep the portable
    x86-64-v3 build; -ffp-contract=off keeps the arithmetic identical.  Returns the flag used."""
    if _NATIVE["built"] is None:
        import tempfile
        out = os.path.join(tempfile.mkdtemp(prefix="orbref_native_"), "liborbref_native.so")
        try:
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "native", "NATIVE_OUT=" + out],
                           check=True, capture_output=True, timeout=120)
            os.environ["ORBREF_LIB"] = out
            _NATIVE["built"] = "-O3 -march=native"
        except Exception as e:   # no compiler: the prebuilt portable copy
            log("native oracle build failed (%s); CPU baseline uses the x86-64-v3 build" % e)
            _NATIVE["built"] = "-O3 -march=x86-64-v3 (native build failed)"
    return _NATIVE["built"]


def cpu_baseline(frames: np.ndarray, budget_s: float):
    """Oracle (scalar C restatement of the reference, 1 thread) on a bounded sample."""
    flags = native_oracle()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orbref
    p = orbref.make_params(NFEAT, SCALE, NLEVELS, INI, MINTH)
    t0 = time.perf_counter()
    prev = None
    n = 0
    for i in range(len(frames)):
        r = orbref.extract(frames[i], p, want_pyramid=False)
        if prev is not None:
            orbref.search_for_initialization(prev.keypoints, prev.descriptors, r.keypoints, r.descriptors, W, H,
                                             window=WINDOW, nnratio=NNRATIO, check_ori=True)
        prev = r
        n += 1
        if time.perf_counter() - t0 >= budget_s:
            break
    dt = time.perf_counter() - t0
    model = ""
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        model = next((l.split(":", 1)[1].strip() for l in out.splitlines() if l.startswith("Model name")), "")
    except Exception:
        pass
    return {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": "oracle/orbref scalar C restatement (%s), frames 0..%d of the config-2 "
                      "sequence, extract + SearchForInitialization(t-1,t), 1 thread, %.1f s" % (flags, n - 1, dt),
            "host_cpu": model or platform.processor(), "host_threads": os.cpu_count()}


def cpu_topology():
    """The CPUs this process may run on (its affinity mask: the box's share) and the host's physical layout
    from sysfs: per allowed CPU its (package, core) pair, so threads can be placed one per physical core."""
    allowed = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))

    def core_of(c):
        base = "/sys/devices/system/cpu/cpu%d/topology/" % c
        try:
            return (int(open(base + "physical_package_id").read()), int(open(base + "core_id").read()))
        except (OSError, ValueError):
            return (0, c)

    cores = {}
    for c in allowed:
        cores.setdefault(core_of(c), []).append(c)
    host_cpus = os.cpu_count() or len(allowed)
    host_cores = len({core_of(c) for c in range(host_cpus)})
    info = {"allowed_cpus": len(allowed), "allowed_physical_cores": len(cores), "host_cpus": host_cpus,
            "host_physical_cores": host_cores}
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for l in out.splitlines():
            k, _, v = l.partition(":")
            if k.strip() in ("Model name", "Socket(s)", "Core(s) per socket", "Thread(s) per core"):
                info[k.strip()] = v.strip()
    except Exception:
        pass
    # the job's CPU quota (cgroup v2 cpu.max "quota period"): the box shares the host by time, not by mask
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        info["cgroup_cpu_quota"] = None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        info["cgroup_cpu_quota"] = None
    # one CPU per physical core first, then the SMT siblings; and the cores that have both siblings allowed,
    # as sibling pairs (for the SMT gain)
    order = [cs[0] for cs in cores.values()] + [c for cs in cores.values() for c in cs[1:]]
    pairs = [c for cs in cores.values() if len(cs) >= 2 for c in cs[:2]]
    return info, order, pairs


def cpu_baseline_all_cores(frames: np.ndarray, budget_s: float, threads: int = 16, pin=None):
    """`threads` workers, each with its own contiguous block of the sequence
    (extract + SearchForInitialization within the block), the oracle's C calls release the GIL.
    pin: CPU ids, worker w pins itself to pin[w] (one per physical core before SMT siblings)."""
    import threading
    flags = native_oracle()
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orbref
    p = orbref.make_params(NFEAT, SCALE, NLEVELS, INI, MINTH)
    done = [0] * threads
    t0 = time.perf_counter()

    def work(w):
        if pin is not None and hasattr(os, "sched_setaffinity"):
            try:
                os.sched_setaffinity(0, {pin[w % len(pin)]})   # the calling thread only (Linux)
            except OSError:
                pass
        prev = None
        i = w * (len(frames) // threads)
        while time.perf_counter() - t0 < budget_s:
            r = orbref.extract(frames[i % len(frames)], p, want_pyramid=False)
            if prev is not None:
                orbref.search_for_initialization(prev.keypoints, prev.descriptors, r.keypoints, r.descriptors, W, H,
                                                 window=WINDOW, nnratio=NNRATIO, check_ori=True)
            prev = r
            done[w] += 1
            i += 1

    ts = [threading.Thread(target=work, args=(w,)) for w in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    return {"value": sum(done) / dt, "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": "oracle/orbref (%s), %d threads each on its own block of the config-2 sequence, extract + "
                      "SearchForInitialization(t-1,t), %d frames in %.1f s%s" % (
                          flags, threads, sum(done), dt, ", pinned one per physical core first" if pin else "")}


def cpu_scaling(frames: np.ndarray, budget_s: float, max_threads: int):
    """the port's thread-scaling curve on this process's CPU share (threads pinned one per
    physical core, then onto SMT siblings), and the all-core figure it grounds: the per-core rate at the
    widest one-thread-per-core point x the host's physical cores x the measured SMT gain (1.0 when the
    share holds no sibling pairs).  Still an extrapolation past the share, labelled as one."""
    info, order, pairs = cpu_topology()
    ncore = info["allowed_physical_cores"]
    pts = sorted({t for t in (1, 2, 4, 8, 16, ncore, len(order), max_threads) if 1 <= t <= min(max_threads, len(order))})
    curve = []
    for t in pts:
        r = cpu_baseline_all_cores(frames, budget_s, t, pin=order)
        curve.append({"threads": t, "frames_per_s": round(r["value"], 2),
                      "physical_cores_used": min(t, ncore)})
    by_t = {c["threads"]: c["frames_per_s"] for c in curve}
    p_core = max(t for t in by_t if t <= ncore)
    per_core = by_t[p_core] / p_core
    # SMT gain inside the job's quota: max_threads threads on max_threads / 2 cores' sibling pairs against
    # max_threads / 2 threads on those cores alone
    smt = None
    h = max_threads // 2
    if h >= 1 and len(pairs) >= 2 * h:
        r_pair = cpu_baseline_all_cores(frames, budget_s, 2 * h, pin=pairs[:2 * h])["value"]
        r_one = by_t[h] if h in by_t else cpu_baseline_all_cores(frames, budget_s, h, pin=pairs[0:2 * h:2])["value"]
        smt = r_pair / r_one
        curve.append({"threads": 2 * h, "frames_per_s": round(r_pair, 2), "physical_cores_used": h,
                      "smt_siblings": True})
    eff = by_t[p_core] / (p_core * by_t[1])
    host_cores = info["host_physical_cores"]
    grounded = per_core * host_cores * (smt if smt else 1.0)
    return {"topology": info, "curve": curve, "parallel_efficiency_at_%d_cores" % p_core: round(eff, 3),
            "smt_gain": round(smt, 3) if smt else None,
            "all_core_grounded": {
                "value": round(grounded, 1), "unit": "frames/s", "cores": host_cores, "kind": "port, extrapolated",
                "sample": "per-core rate at %d pinned threads (%.2f frames/s/core, parallel efficiency %.2f vs 1 thread) "
                          "x %d physical cores x SMT gain %s: NOT MEASURED on the whole host (the box gives one "
                          "GPU's job a %d-CPU share)" % (p_core, per_core, eff, host_cores,
                                                         ("%.2f (measured on %d sibling pairs)" % (smt, h)) if smt else
                                                         "1.0 (no sibling pairs allowed)",
                                                         info.get("cgroup_cpu_quota") or info["allowed_cpus"])}}


DUMP_SAMPLE_BYTES = 48 << 20   # the per-keypoint arrays of --dump-outputs together (64 MB is the limit for all files)


def dump_outputs(path, pl, m12, nm):
    """--dump-outputs: what one step hands its caller, as float32 .npy files under `path`.

    pl is the step's payload (kps int32 (B, cap, 7) = cv::KeyPoint records, desc uint8 (B, cap, 32), counts (B,)),
    m12 / nm its SearchForInitialization result for the pairs (f, f + 1).  The per-keypoint arrays of a whole batch
    are far larger than the limit, so they are written for a fixed seeded sample of frames (sample_frames.npy, the
    same for every run with the same --batch); counts and nmatches are written whole.  Slots at or past a frame's
    count hold whatever an earlier batch left there: they are written as 0 (matches12: -1).
      keypoints.npy    (n, cap, 7)   x, y, size, angle, response, octave, class_id of frame sample_frames[i]
      descriptors.npy  (n, cap, 32)  descriptor bytes
      matches12.npy    (n, cap)      vnMatches12 of the pair (sample_frames[i], sample_frames[i] + 1)
      counts.npy (B,), nmatches.npy (B - 1,), sample_frames.npy (n,)"""
    B, cap = pl.kps.shape[0], pl.kps.shape[1]
    dev = pl.kps.device
    n = max(1, min(max(1, B - 1), DUMP_SAMPLE_BYTES // (cap * (7 + 32 + 1) * 4)))
    idx = np.sort(np.random.default_rng(0).choice(max(1, B - 1), size=n, replace=False))
    it = torch.from_numpy(idx).to(dev)
    valid = torch.arange(cap, device=dev)[None, :] < pl.counts[it].to(torch.int64)[:, None]
    k = pl.kps[it]
    kf = torch.cat([k[..., :5].contiguous().view(torch.float32), k[..., 5:].to(torch.float32)], dim=2)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    arrays = {
        "keypoints": torch.where(valid[..., None], kf, zero),
        "descriptors": torch.where(valid[..., None], pl.desc[it].to(torch.float32), zero),
        "counts": pl.counts.to(torch.float32),
        "nmatches": nm.to(torch.float32),
        "sample_frames": it.to(torch.float32),
    }
    if B > 1:
        arrays["matches12"] = torch.where(valid, m12[it].to(torch.float32), zero - 1)
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")),
                    help="ranks (one per GPU); without a launcher, N > 1 starts them through torch.distributed.run")
    ap.add_argument("--dry-run", action="store_true", help="print the launch plan and exit")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="frames per GPU per step (round 6, K = 20, "
                    "tools/diag/batch_stream_sweep.sh: three streams 768 -> 279.0k, 1024 -> 281.1-283.0k, 1536 -> 283.5k, "
                    "2048 -> 286.5-290.2k, 4096 -> 287.0-288.3k frames/s; two streams 2048 -> 286.8k, 4096 -> "
                    "290.1-295.3k, 6144 -> 290.2k, 8192 -> 288.3k: the pipeline's fill and drain and the fixed "
                    "per-launch costs weigh less, and two batches in flight share the CUs and caches better than three)")
    ap.add_argument("--pool", type=int, default=2, help="distinct batches resident per GPU (2 x 4096 frames = 3.8 GB > the 256 MB Infinity Cache)")
    ap.add_argument("--streams", type=int, default=2, help="pipeline depth (batches in flight per GPU; "
                    "GPU_MAX_HW_QUEUES=4 leaves 3 besides the default stream; at 4096 frames per step 2 beat 3: "
                    "290.1-295.3k against 287.0-288.3k frames/s)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run the instrumented and isolated passes (stage times, rooflines), "
                         "the copy-bandwidth probe, the rank-0 ingress proxy, the host-fed leg and the CPU baselines; "
                         "the options below that size those legs only matter with it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy, see dump_outputs()")
    ap.add_argument("--iso-steps", type=int, default=3, help="untimed one-stream steps for roofline_isolated")
    ap.add_argument("--match-stream", action="store_true",
                    help="SearchForInitialization on the default stream beside the extraction streams")
    ap.add_argument("--instrument-timed", action="store_true",
                    help="record the per-stage events inside the timed region (default: a separate pass)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=16,
                    help="threads of the all-core CPU figure (the box's CPU share is 16 per GPU)")
    ap.add_argument("--ingress-peers", type=int, default=7,
                    help="N = 1 only: peers whose hand-back the rank-0 ingress proxy copies per step (0 = skip)")
    ap.add_argument("--host-steps", type=int, default=60,
                    help="timed steps of the host-fed leg (frames from pinned host memory, uploaded on a copy "
                         "stream overlapped with the previous batches' extraction); 0 = skip")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:   # launch_plan already refused this; kept for imports of main()
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    torch.cuda.set_device(local)   # before the process group, so RCCL binds this rank's GPU
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        world = dist.get_world_size()
    dev = torch.device("cuda", local)
    B = args.batch
    nb = max(1, args.pool)

    # synthetic KITTI replay: each rank owns its own contiguous block of the sequence
    seq = orbx_synth.kitti_sequence(B * nb, start=rank * B * nb)
    frames = torch.from_numpy(seq).to(dev)
    # P-deep pipeline: step k runs on stream k % P with its own extractor workspace and
    # payload, so the latency-bound stages of one batch (quadtree, greedy matching) overlap
    # the throughput-bound stages of the next; each stream stays in order
    # (extract -> match -> gather).
    P = max(1, args.streams)
    exs = [orbx.ORBextractor(NFEAT, SCALE, NLEVELS, INI, MINTH, device=local) for _ in range(P)]
    ex = exs[0]
    cap = ex.capacity(H, W)
    # each slot double-buffers its payload: batch k's hand-back to rank 0 overlaps batch k+1's extraction
    hands = [orbx_dist.HandBack(B, cap, dev, world, rank) for _ in range(P)]
    last_payload = [None]
    matcher = orbx.ORBmatcher(NNRATIO, True)
    pa = torch.arange(0, B - 1, dtype=torch.int32, device=dev)
    pb = torch.arange(1, B, dtype=torch.int32, device=dev)
    m12 = [torch.empty((B - 1, cap), dtype=torch.int32, device=dev) for _ in range(P)]
    nm = [torch.empty((B - 1,), dtype=torch.int32, device=dev) for _ in range(P)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(P)]
    # --match-stream: SearchForInitialization of every batch on the default stream (a hardware queue of its
    # own), ordered after its batch's extraction by an event, so the extraction streams do not wait for it
    mstream = torch.cuda.default_stream(dev) if args.match_stream else None
    pl_done = {}   # payload -> event after the last match that read it
    ev_m = []

    def step(k, timed=False, j=None):
        base = (k % nb) * B
        j = k % P if j is None else j
        s = streams[j]
        with torch.cuda.stream(s):
            pl = hands[j].next_payload()
        if mstream is not None and id(pl) in pl_done:
            s.wait_event(pl_done[id(pl)])   # the match that read this payload is done before it is rewritten
        exs[j].extract_batch_device(frames[base:base + B], pl.kps, pl.desc, pl.counts, s)
        ms = s
        if mstream is not None:
            ex_done = torch.cuda.Event()
            ex_done.record(s)
            mstream.wait_event(ex_done)
            ms = mstream
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ms)
        matcher.search_for_initialization_batch(pl.kps, pl.desc, pl.counts, pa, pb, H, W, WINDOW, m12[j], nm[j], ms)
        if timed:
            e1.record(ms)
            ev_m.append((e0, e1))
        if mstream is not None:
            d = torch.cuda.Event()
            d.record(mstream)
            pl_done[id(pl)] = d
        with torch.cuda.stream(s):
            hands[j].send()
        last_payload[0] = pl

    for k in range(args.warmup):
        step(k)
    for j in range(P):
        exs[j].sync(streams[j])
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # The timed region runs the pipeline as a user would, without instrumentation: the per-stage event
    # pairs (5 per extract, 2 per match) cost about 2% of the rate; the pipelined stage breakdown comes
    # from a second, instrumented pass of the same steps below (--instrument-timed: events in the timed
    # region, the round-1/2 behaviour)
    inst = args.instrument_timed
    for e in exs:
        e.set_timing(inst)
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(args.warmup + k, timed=inst)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    for j in range(P):
        exs[j].sync(streams[j])   # raises on device-side overflow
    elapsed = t1 - t0
    # results of the last timed step, read now: the host-fed leg below reuses the payloads and m12 / nm
    jl = (args.warmup + args.steps - 1) % P
    counts = last_payload[0].counts.cpu().numpy()
    nmatch = nm[jl].cpu().numpy()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_payload[0], m12[jl], nm[jl])
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    used = sorted({(args.warmup + k) % P for k in range(args.steps)})
    full = args.full
    elapsed_inst = None
    if full and not inst:   # the instrumented pass (not part of `value`)
        for e in exs:
            e.set_timing(True)
        torch.cuda.synchronize()
        ti = time.perf_counter()
        for k in range(args.steps):
            step(args.warmup + k, timed=True)
        torch.cuda.synchronize()
        elapsed_inst = time.perf_counter() - ti
        for j in range(P):
            exs[j].sync(streams[j])
    stage_ms, match_ms = None, None
    if full or inst:
        stage_ms = sum(exs[j].stage_times() for j in used)   # sums over the instrumented steps (all streams)
        match_ms = sum(a.elapsed_time(b) for a, b in ev_m)

    # isolated pass (after the timed region, not part of `value`): the same steps one at a
    # time on one stream, so every kernel's duration is its own (roofline_isolated)
    iso_stage, iso_match = None, None
    if full and args.iso_steps > 0 and P > 1:
        ev_m.clear()
        exs[0].set_timing(True)
        for k in range(args.iso_steps):
            step(k, timed=True, j=0)
        torch.cuda.synchronize()
        exs[0].sync(streams[0])
        iso_stage = exs[0].stage_times() / args.iso_steps
        iso_match = sum(a.elapsed_time(b) for a, b in ev_m) / args.iso_steps

    # Rank-0 ingress proxy (not part of `value`): at N = 8, rank 0 takes in 7 peers'
    # hand-back payloads per step while it extracts its own frames.  On one GPU, the same pipeline runs with a
    # side stream that, once step k's extraction is done, copies the step's payload size `peers` times
    # device-to-device into receive buffers -- the local HBM reads and writes, and the CU time, of RCCL's
    # receive path when it lands a peer's data in a staging buffer and copies it out (a direct P2P write
    # would only add the writes, so this bounds the cost from above).
    ingress = None
    if full and world == 1 and args.ingress_peers > 0:
        nbp = hands[0].payloads[0].nbytes
        rbuf = [torch.empty(nbp, dtype=torch.uint8, device=dev) for _ in range(args.ingress_peers)]
        src = torch.empty(nbp, dtype=torch.uint8, device=dev)
        src.fill_(7)
        side = torch.cuda.Stream(device=dev)
        for e in exs:
            e.set_timing(False)

        def istep(k):
            step(k)
            ev = torch.cuda.Event()
            ev.record(streams[k % P])
            side.wait_event(ev)
            with torch.cuda.stream(side):
                for r in rbuf:
                    r.copy_(src)

        for k in range(min(args.warmup, 2 * P)):
            istep(k)
        torch.cuda.synchronize()
        i0 = time.perf_counter()
        for k in range(args.steps):
            istep(args.warmup + k)
        torch.cuda.synchronize()
        ielapsed = time.perf_counter() - i0
        for j in range(P):
            exs[j].sync(streams[j])
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):   # the copies alone, on an idle GPU
            c0.record(side)
            for _ in range(4):
                for r in rbuf:
                    r.copy_(src)
            c1.record(side)
        torch.cuda.synchronize()
        copy_ms = c0.elapsed_time(c1) / 4
        ingress = {"peers": args.ingress_peers, "bytes_per_step": nbp * args.ingress_peers,
                   "value": round(B * args.steps / ielapsed, 2), "unit": "frames/s",
                   "ms_per_step": round(ielapsed / args.steps * 1e3, 4),
                   "copies_alone_ms_per_step": round(copy_ms, 4),
                   "copies_alone_GBps": round(2 * nbp * args.ingress_peers / (copy_ms * 1e-3) / 1e9, 1),
                   "model": "side-stream device-to-device copies of %d payloads of %d B per step, each step's copies "
                            "ordered after its extraction (upper bound on rank 0's receive cost at N = %d)" % (
                                args.ingress_peers, nbp, args.ingress_peers + 1)}
        del rbuf, src

    # host-fed leg (not part of `value`): the same pipeline, but every batch starts in pinned host
    # memory, as ORBextractor::operator() receives its image (include/ORBextractor.h:58-61).  A copy
    # stream uploads batch k into pipeline slot k % P's input buffer while the other slots extract;
    # slot j's buffer is overwritten only after its previous extraction has finished reading it.
    host_fed = None
    if full and args.host_steps > 0 and world == 1:   # per-GPU PCIe figure; N > 1 ranks would each pin a 3.8 GB copy
        hseq = torch.from_numpy(seq).pin_memory()
        # input ring deeper than the pipeline: an upload may run two batches ahead of the oldest extraction
        # still reading its buffer (a slot's extraction lasts about P step times while it shares the chip)
        R = int(os.environ.get("ORBX_HOST_RING", str(2 * P)))
        dbuf = [torch.empty((B, H, W), dtype=torch.uint8, device=dev) for _ in range(R)]
        # high priority: HIP keeps it off the hardware queues the default-priority compute streams use
        # (GPU_MAX_HW_QUEUES = 4), so an upload never waits behind another slot's kernels
        cstream = torch.cuda.Stream(device=dev, priority=int(os.environ.get("ORBX_COPY_PRIO", "-1")))
        up_done = [torch.cuda.Event() for _ in range(R)]
        ex_done = [torch.cuda.Event() for _ in range(R)]
        for i in range(R):
            ex_done[i].record(streams[i % P])

        def hstep(k):
            base = (k % nb) * B
            j = k % P
            s = streams[j]
            with torch.cuda.stream(s):
                pl = hands[j].next_payload()
            i = k % R
            cstream.wait_event(ex_done[i])
            with torch.cuda.stream(cstream):
                dbuf[i].copy_(hseq[base:base + B], non_blocking=True)
                up_done[i].record(cstream)
            s.wait_event(up_done[i])
            exs[j].extract_batch_device(dbuf[i], pl.kps, pl.desc, pl.counts, s)
            ex_done[i].record(s)
            matcher.search_for_initialization_batch(pl.kps, pl.desc, pl.counts, pa, pb, H, W, WINDOW, m12[j], nm[j],
                                                    s)
            with torch.cuda.stream(s):
                hands[j].send()

        for k in range(min(args.warmup, 2 * P)):
            hstep(k)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        h0 = time.perf_counter()
        for k in range(args.host_steps):
            hstep(k)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        helapsed = time.perf_counter() - h0
        for j in range(P):
            exs[j].sync(streams[j])
        if world > 1:
            tt = torch.tensor([helapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            helapsed = float(tt.item())
        # the upload alone, for the PCIe figure
        u0 = torch.cuda.Event(enable_timing=True)
        u1 = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(cstream):
            u0.record(cstream)
            for k in range(4):
                dbuf[k % R].copy_(hseq[(k % nb) * B:(k % nb) * B + B], non_blocking=True)
            u1.record(cstream)
        torch.cuda.synchronize()
        up_gbs = 4 * B * H * W / (u0.elapsed_time(u1) * 1e-3) / 1e9
        host_fed = {"value": round(world * B * args.host_steps / helapsed, 2), "unit": "frames/s",
                    "steps": args.host_steps, "ms_per_step": round(helapsed / args.host_steps * 1e3, 4),
                    "upload_GBps": round(up_gbs, 1), "upload_ms_per_batch": round(B * H * W / up_gbs / 1e6, 4),
                    "input": "pinned host memory, H2D on a copy stream overlapped with extraction (PCIe-inclusive)"}
        del hseq

    for j in range(P):
        with torch.cuda.stream(streams[j]):
            hands[j].drain()
    torch.cuda.synchronize()

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    K = args.steps
    frames_total = world * B * K
    value = frames_total / elapsed
    # the stage breakdown and the rooflines below need per-stage times: --full or --instrument-timed
    stages = None if stage_ms is None else {
        "pyramid": float(stage_ms[0]) / K, "fast": float(stage_ms[1]) / K, "quadtree": float(stage_ms[2]) / K,
        "describe": float(stage_ms[3]) / K, "match": match_ms / K}
    # algorithmic bytes per launch (DESIGN.md "Roofline"): one launch covers B frames
    sizes = level_sizes()
    A = [w * h for w, h in sizes]
    n_cand = None
    try:
        if stages is not None:
            n_cand = int(sum(len(ex.debug_candidates(0, l)) for l in range(NLEVELS)))
    except Exception:
        pass
    kept = float(counts.mean())
    cand = float(n_cand if n_cand is not None else 10 * NFEAT)
    n_launch = ex.debug_launches(H, W, B)
    alg = {
        # each launch reads its source level once and writes its levels (orbx_debug_launches)
        "pyramid": B * (sum(A[l] for l in range(NLEVELS) if n_launch["pyramid_sources"] >> l & 1) + sum(A[1:])),
        "fast": B * (sum(A) + 4 * cand),
        "quadtree": B * (4 * cand + 4 * kept),
        # compulsory bytes: every level pixel once (patches overlap), the packed keypoint in,
        # the 28 B keypoint + 32 B descriptor out
        "describe": B * (sum(A) + kept * (4 + 60)),
        "match": (B - 1) * 2 * kept * 60,
    }
    def roofline(st):
        dom = max(st, key=lambda k: st[k])
        # several launches of one kernel per stage: per-launch figures are stage / launches,
        # like rocprofv3's per-kernel average (the library reports its launch plan for this batch:
        # pyramid one per level, FAST one per LDS class of cells, orbx_extract.hip)
        launches = {"pyramid": n_launch["pyramid"], "fast": n_launch["fast"]}.get(dom, 1)
        t_launch = st[dom] / launches * 1e-3
        achieved = alg[dom] / launches / t_launch / 1e9
        qk = "k_quadtree"
        kname = {"pyramid": "k_pyramid_level", "fast": "k_fast_cells", "quadtree": qk + "<512,16|512,8|256,4>",
                 "describe": "k_describe", "match": "k_si_grid+k_si_build+k_si_greedy"}[dom]
        # stages made of several kernels: their per-launch counters add up
        PARTS = {"match": ["k_si_grid", "k_si_build", "k_si_greedy"],
                 "quadtree": [qk + "<512, 16", qk + "<512, 8", qk + "<256, 4"]}

        def per_launch(K, dom, kname, field):
            """A counter per launch from a per-kernel table keyed by full names (template arguments
            included): a multi-kernel stage adds one launch of each part; otherwise the average per
            dispatch over every template of the kernel."""
            if dom in PARTS:
                return sum(sum(K[k][field] for k in K if k == p or k.startswith(p + "<") or
                               (p.endswith(tuple("0123456789")) and k.startswith(p + ","))) for p in PARTS[dom])
            ks = [k for k in K if k == kname or k.startswith(kname + "<")]
            nd = sum(K[k]["dispatches"] for k in ks)
            return sum(K[k][field] * K[k]["dispatches"] for k in ks) / nd
        # HBM bytes per launch from the committed rocprofv3 FETCH_SIZE/WRITE_SIZE passes of this
        # same command (tools/collect_pmc.sh -> tools/pmc_summary.py); null when absent
        # Both counter files carry the kernel-source hash of the tree they were measured on; a file from
        # another tree is reported as stale and its figures are not used.
        traffic = None
        src_sha = kernel_sources_sha256()
        counters = {"kernel_sources_sha256": src_sha}
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc):
            try:
                d = json.load(open(pmc))
                counters["pmc_traffic_sha256"] = d.get("kernel_sources_sha256")
                if d.get("batch") == B and d.get("kernel_sources_sha256") == src_sha:
                    traffic = int(per_launch(d["kernels"], dom, kname, "bytes_per_launch"))
            except Exception:
                traffic = None
        r = {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
             "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
             "alg_bytes_per_launch": int(alg[dom] / launches), "launch_ms": round(t_launch * 1e3, 4)}
        # the path is integer VALU work: issue rate of the same kernel against the VALU peak
        # (256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per wave64 instruction), instruction count from
        # the committed SQ_INSTS_VALU pass (tools/gpu_sq.sh -> profiles/sq_counters.json)
        sq = os.path.join(ROOT, "profiles", "sq_counters.json")
        if os.path.exists(sq):
            try:
                d = json.load(open(sq))
                counters["sq_counters_sha256"] = d.get("kernel_sources_sha256")
                if d.get("batch") == B and d.get("kernel_sources_sha256") == src_sha:
                    ins = per_launch(d["per_dispatch_averages"], dom, kname, "SQ_INSTS_VALU")
                    rate = ins / t_launch / 1e9
                    pk, pins, p2 = valu_peak(kname)
                    r["valu_issue"] = {
                        "insts_per_launch": int(ins), "achieved": round(rate, 1), "peak": pk,
                        "unit": "G wave-instr/s", "frac": round(rate / pk, 4),
                        "peak_basis": "measured issue rate of %s, 8 waves/SIMD (profiles/r02/valu_rate.json)" % pins,
                        "peak_2cycle_ops": p2,
                        "note": "an issue ratio against the rate of the kernel's slowest (4-cycle) dominant "
                                "instruction: an upper bound on how issue-bound the kernel is, not proof that the "
                                "VALU pipe is its limiter (DESIGN.md section 6)"}
            except Exception:
                pass
        counters["current"] = (counters.get("pmc_traffic_sha256") == src_sha and
                               counters.get("sq_counters_sha256") == src_sha)
        r["counters"] = counters
        return r

    out = {
        "metric": BASELINE["metric"],
        "value": round(value, 2),
        "unit": "frames/s",
        "n_gpus": world,
        "world_size": world,
        "steps": K,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / K * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (seeded KITTI-like 1241x376 replay, orb-slam-_amd/orbx_synth.py)",
        "config": {"workload": "config2_kitti_1241x376_2000feat_8lv_s1.2_extract+SearchForInitialization",
                   "frames_per_gpu_per_step": B, "batches_in_flight": P, "parallelism": "frames sharded, gather to rank 0" if world > 1
                   else "single GPU", "pairs_per_gpu_per_step": B - 1, "window": WINDOW,
                   "input": "device-resident (frames in HBM before the timed region; host-fed figure in "
                            "value_host_fed)",
                   "handback_bytes_per_rank_per_step": hands[0].payloads[0].nbytes,
                   "handback_bytes_to_rank0_per_step": hands[0].payloads[0].nbytes * (world - 1)},
        "keypoints_per_frame": round(kept, 1),
        "matches_per_pair": round(float(nmatch.mean()), 1),
    }
    if stages is not None:
        out["stage_ms_per_step"] = {k: round(v, 4) for k, v in stages.items()}
        out["stage_timing"] = ("per-stage HIP events in the timed region" if elapsed_inst is None else
                               "per-stage HIP events in a second pass of the same steps (%.1f frames/s with the events)"
                               % (world * B * K / elapsed_inst))
        out["roofline"] = roofline(stages)
    if host_fed is not None:
        out["value_host_fed"] = host_fed["value"]
        out["host_fed"] = host_fed
    if ingress is not None:
        ingress["vs_value"] = round(ingress["value"] / value, 4)
        out["rank0_ingress_proxy"] = ingress
    if iso_stage is not None:
        # Kernel rooflines come from the one-stream pass: under the P-deep pipeline a kernel
        # shares the CUs with the other streams' kernels and its event interval also holds
        # queueing, so only the isolated durations describe the kernel itself (and agree
        # with rocprofv3 --kernel-trace of `bench.py --streams 1`).  The pipelined figures
        # stay alongside.
        iso = {"pyramid": float(iso_stage[0]), "fast": float(iso_stage[1]), "quadtree": float(iso_stage[2]),
               "describe": float(iso_stage[3]), "match": iso_match}
        out["stage_ms_isolated"] = {k: round(v, 4) for k, v in iso.items()}
        out["roofline_pipelined"] = out["roofline"]
        out["roofline"] = dict(roofline(iso), timing="isolated one-stream pass after the timed region "
                                                        "(same batches); see roofline_pipelined")
    if full:
        try:   # after the timed region; not part of `value`
            cbw, cinfo = copy_bandwidth(dev)
            out["roofline"]["hbm_copy_GBps"] = round(cbw, 1)
            out["roofline"]["hbm_copy"] = cinfo
            out["roofline"]["frac_of_copy"] = round(out["roofline"]["achieved"] / cbw, 5)
        except Exception:
            pass
    if full and world == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(seq, args.cpu_seconds)
        out["speedup_vs_cpu"] = round(value / out["cpu_baseline"]["value"], 1)
        if args.cpu_threads > 1:
            # SURVEY 8d (ii) asks for nproc workers.  The GPU box gives one GPU's job a 16-CPU share
            # (os.cpu_count() shows the whole host): the thread-scaling curve is measured on the share, pinned
            # one thread per physical core before SMT siblings, and the whole-host figure is grounded on it
            sc = cpu_scaling(seq, args.cpu_seconds / 3, args.cpu_threads)
            top = max((c for c in sc["curve"] if not c.get("smt_siblings")), key=lambda c: c["threads"])
            out["cpu_baseline_all_cores"] = {
                "value": top["frames_per_s"], "unit": "frames/s", "cores": top["threads"], "kind": "port",
                "sample": "oracle/orbref (%s), %d pinned threads each on its own block of the config-2 sequence, "
                          "extract + SearchForInitialization(t-1,t), %.1f s" % (native_oracle(), top["threads"],
                                                                               args.cpu_seconds / 3)}
            out["speedup_vs_cpu_all_cores"] = round(value / top["frames_per_s"], 1)
            out["cpu_scaling"] = sc
            g = sc["all_core_grounded"]["value"]
            out["speedup_vs_cpu_all_core_grounded"] = round(value / g, 1)
            out["target_50x"] = {
                "vs_1_thread": value / out["cpu_baseline"]["value"] >= 50.0,
                "vs_all_core_grounded": value / g >= 50.0,
                "note": "BASELINE north_star: >= 50x the reference CPU ORBextractor+ORBmatcher throughput on 1 "
                        "MI355X; figure (i) 1 thread per image, figure (ii) all cores (SURVEY 8d).  The CPU side "
                        "is the scalar orbref port, not OpenCV's SIMD build"}
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
