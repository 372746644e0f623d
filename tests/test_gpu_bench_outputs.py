"""bench.py's plain and --full runs on a small batch: the result line of a plain run carries the headline figure
and nothing that takes passes of its own, `--steps` sets the timed steps, `--dump-outputs` writes what the last
timed step computed (checked against an extraction and a SearchForInitialization of the same frames in this
process, and slot by slot against the counts), and `--full` still brings the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
B, STEPS, WARMUP = 6, 3, 1
SMALL = ["--gpus", "1", "--batch", str(B), "--pool", "2", "--steps", str(STEPS), "--warmup", str(WARMUP)]
MOVED = ("stage_ms_per_step", "stage_ms_isolated", "roofline", "roofline_pipelined", "host_fed", "value_host_fed",
         "rank0_ingress_proxy", "cpu_baseline", "cpu_scaling", "speedup_vs_cpu")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench(SMALL + ["--dump-outputs", str(d)]), d


def test_plain_line(plain):
    line, _ = plain
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same STEPS steps of B frames
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / B - 1.0) < 1e-3
    assert not [k for k in MOVED if k in line]


def test_dumped_outputs_are_the_last_steps_results(plain, cuda):
    import torch

    import orbx
    import orbx_synth
    _, d = plain
    arr = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(arr) == ["counts", "descriptors", "keypoints", "matches12", "nmatches", "sample_frames"]
    assert all(a.dtype == np.float32 for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    # the last timed step (k = WARMUP + STEPS - 1) reads batch k % pool of the replay
    base = ((WARMUP + STEPS - 1) % 2) * B
    frames = torch.from_numpy(orbx_synth.kitti_sequence(B, start=base)).to(cuda)
    ex = orbx.ORBextractor(2000, 1.2, 8, 20, 7, device=0)
    cap = ex.capacity(376, 1241)
    kps = torch.zeros((B, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.zeros((B,), dtype=torch.int32, device=cuda)
    ex.extract_batch_device(frames, kps, desc, counts)
    pa = torch.arange(0, B - 1, dtype=torch.int32, device=cuda)
    m12, nm = orbx.ORBmatcher(0.9, True).search_for_initialization_batch(kps, desc, counts, pa, pa + 1, 376, 1241, 100)
    ex.sync(torch.cuda.current_stream())
    cnt = counts.cpu().numpy()
    assert cnt.min() > 1500
    assert np.array_equal(arr["counts"], cnt.astype(np.float32))
    assert np.array_equal(arr["nmatches"], nm.cpu().numpy().astype(np.float32))
    idx = arr["sample_frames"].astype(np.int64)
    assert np.array_equal(idx, np.arange(B - 1))     # a batch this small fits whole
    assert arr["keypoints"].shape == (B - 1, cap, 7) and arr["descriptors"].shape == (B - 1, cap, 32)
    assert arr["matches12"].shape == (B - 1, cap)
    klist = orbx.keypoints_from_device(kps, counts)
    dh, mh = desc.cpu().numpy(), m12.cpu().numpy()
    for i, f in enumerate(idx):
        n = cnt[f]
        for c, fld in enumerate(("x", "y", "size", "angle", "response", "octave", "class_id")):
            assert np.array_equal(arr["keypoints"][i, :n, c], klist[f][fld].astype(np.float32)), (f, fld)
        assert np.array_equal(arr["descriptors"][i, :n], dh[f, :n].astype(np.float32))
        assert np.array_equal(arr["matches12"][i, :n], mh[i, :n].astype(np.float32))
        assert not arr["keypoints"][i, n:].any() and not arr["descriptors"][i, n:].any()
        assert (arr["matches12"][i, n:] == -1).all()


def test_full_run_brings_the_other_legs(cuda):
    line = _bench(SMALL + ["--full", "--no-cpu", "--host-steps", "2"])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    for k in ("stage_ms_per_step", "stage_ms_isolated", "roofline", "roofline_pipelined", "host_fed",
              "rank0_ingress_proxy"):
        assert k in line, k
    assert "hbm_copy_GBps" in line["roofline"]
