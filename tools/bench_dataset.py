#!/usr/bin/env python3
"""A training batch from the device-resident dataset (pmoe_amd/data.py) against the path it replaces, at the headline shape: a
store of 4096 frames of 256 x 256, B = 64 windows of T = 4 frames.
  python tools/bench_dataset.py [--frames 4096] [--size 256] [--batch 64] [--calls 200] [--rounds 7] [--warmup 3]
                                [--ingest-frames 128] [--json out.json]
Times, per batch:
  (a) ds.batch(ids) in val mode: one gather + ToTensor launch, one gather of the measurement rows
  (b) ds.batch(ids) in train mode, super_hard at iteration 64000: gather into a uint8 staging tensor + the augmenter's launches
  (b2) the same with one drawn plan reused for every batch: (b) without the host's plan draw, which otherwise paces the device
  (c) the parent path: pre(raw [64, 4, 600, 800, 3], augment=get_augmenter(64000, 64, "super_hard")) from raw frames already
      on the device -- the call tools/bench_augment.py times (the reference's loader would first decode and upload them)
as device time (events around `calls` calls) and wall time (host clock around the same calls, ending in a synchronise), after a
warm-up, (a), (b), (b2), (c) alternating inside each round of one process; the median over the rounds with [min .. max].
Also the ingest rate in frames/s of decode (PIL, thread pool) + upload (pinned chunks) + resize for a directory of
`--ingest-frames` synthetic 600 x 800 PNGs written to a temporary directory (0: skipped; skipped too without PIL)."""
import argparse
import copy
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmoe_amd import data, hip                                           # noqa: E402
from pmoe_amd.augment import get_augmenter                               # noqa: E402
from pmoe_amd.preprocess import FramePreprocessor                        # noqa: E402

H0, W0, CROP, T, EPISODES = 600, 800, (125, 90), 4, 8


def _ingest_rate(n, size):
    """frames/s of CarlaSegPred(root) over n synthetic PNGs (blocks + low-order noise: neither flat nor incompressible)"""
    try:
        from PIL import Image
    except ImportError:
        return None
    import numpy as np
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        for sub in ("rgb", "measurements"):
            (root / "ep0" / sub).mkdir(parents=True)
        for i in range(n):
            coarse = rng.integers(0, 256, (H0 // 8, W0 // 8, 3), dtype=np.uint8)
            img = np.repeat(np.repeat(coarse, 8, 0), 8, 1) ^ rng.integers(0, 8, (H0, W0, 3), dtype=np.uint8)
            Image.fromarray(img).save(root / "ep0" / "rgb" / f"{i:05d}.png", compress_level=1)
            (root / "ep0" / "measurements" / f"{i:05d}.json").write_text(json.dumps(
                dict(steer=0.0, brake=0.0, throttle=0.5, speed=5.0, target_speed=6.0, command=1 + i % 4)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = data.CarlaSegPred(str(root), past_frames=T, future_frames=0, mode="val", load_measurements=True,
                               crop=CROP, resize=(size, size))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(ds.store) == n
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ingest-frames", type=int, default=128)
    ap.add_argument("--json", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset: needs the MI355X (no CPU path, no CPU timing)")
    torch.manual_seed(0)
    per = a.frames // EPISODES
    records = [dict(steer=0.1, brake=0.0, throttle=0.5, speed=5.0 + (k % 7), target_speed=6.0, command=1 + k % 4) for k in range(per)]
    t0 = time.perf_counter()
    episodes = [dict(rgb=torch.randint(0, 256, (per, H0, W0, 3), dtype=torch.uint8, device="cuda"), measurements=records)
                for _ in range(EPISODES)]
    train = data.CarlaSegPred.from_arrays(episodes, T, 0, aug_type="super_hard", mode="train", load_measurements=True,
                                          batch_size=a.batch, boost=1, crop=CROP, resize=(a.size, a.size))
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0
    raw = episodes[0]["rgb"][:a.batch * T].view(a.batch, T, H0, W0, 3).clone()      # what (c) starts from
    del episodes
    train.samples_read = 64000                                          # the schedule of get_augmenter(64000, 64, "super_hard")
    val = copy.copy(train)                                              # the same store, the other mode
    val.mode = "val"
    pre = FramePreprocessor(CROP, (a.size, a.size))
    aug = get_augmenter(64000, a.batch, "super_hard")
    gen = torch.Generator().manual_seed(1)
    fixed = aug.plan(a.batch * T, a.size, a.size, generator=torch.Generator().manual_seed(3))   # (b2: no host draw per batch)
    order = torch.randperm(len(train), generator=torch.Generator().manual_seed(2))
    cursor = [0]

    def ids():
        k = cursor[0]
        cursor[0] = (k + a.batch) % (len(train) - a.batch)
        return order[k:k + a.batch]

    variants = [("a: val batch", lambda: val.batch(ids())),
                ("b: train batch, super_hard @ 64000", lambda: train.batch(ids(), generator=gen)),
                ("b2: train batch, one plan reused", lambda: train.batch(ids(), plan=fixed)),
                ("c: parent pre(raw, augment)", lambda: pre(raw, augment=aug, generator=gen))]
    launches = {}
    for name, call in variants:
        for _ in range(a.warmup):
            call()
        with hip.LaunchRecorder() as rec:
            call()
        launches[name] = len(rec.calls)
    torch.cuda.synchronize()
    wall = {name: [] for name, _ in variants}
    devt = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, call in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
            devt[name].append(e0.elapsed_time(e1) / a.calls)
    print(f"store of {len(train.store)} frames {a.size} x {a.size} ({len(train.store) * train.store.row_bytes / 1e6:.0f} MB, filled from "
          f"device frames in {fill_s:.1f} s), {len(train)} windows; B = {a.batch}, T = {T}; {a.calls} calls per window, "
          f"{a.rounds} rounds (median [min .. max])")
    out = {"frames": len(train.store), "size": a.size, "batch": a.batch, "T": T, "calls": a.calls, "rounds": a.rounds, "variants": {}}
    for name, _ in variants:
        w, d = wall[name], devt[name]
        print(f"  {name:36s} device {statistics.median(d):7.3f} ms [{min(d):.3f} .. {max(d):.3f}]   "
              f"wall {statistics.median(w):7.3f} ms [{min(w):.3f} .. {max(w):.3f}]   {launches[name]} launches (last warm call)")
        out["variants"][name.split(":")[0]] = {"what": name, "device_ms": [statistics.median(d), min(d), max(d)],
                                               "wall_ms": [statistics.median(w), min(w), max(w)], "launches": launches[name]}
    rate = _ingest_rate(a.ingest_frames, a.size) if a.ingest_frames > 0 else None
    print("  ingest (decode + upload + resize): " + (f"{rate:.0f} frames/s over {a.ingest_frames} PNGs of {H0} x {W0}, "
                                                      f"{data.cpu_share()} decode threads" if rate else "not measured"))
    out["ingest_frames_per_s"] = rate
    out["ingest_threads"] = data.cpu_share()
    print(json.dumps(out))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
