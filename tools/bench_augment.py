#!/usr/bin/env python3
"""Input pipeline with and without the train-time augmenter: 256 camera frames of 600 x 800 -> 256 x 256 (the 64 x 4 frames one
headline step consumes).
  python tools/bench_augment.py [--frames 256] [--size 256] [--calls 20] [--rounds 5] [--warmup 3]
Prints, per variant, the time of one call:
  (a) pre(frames)                                                          Crop -> Resize -> ToTensor, 2 launches
  (b) pre(frames, augment=get_augmenter(64000, 64, "super_hard"))           + a fresh plan per call
  (c) pre(frames, augment=get_augmenter(aug_type="segmentation"))
as wall time (host clock around `calls` calls that end in a synchronise: what a training loop pays, the host's plan draw
included) and as device time (events around the same calls), the median over `rounds` rounds with the variants alternating
inside each round, plus the host-only time of Augmenter.plan and the launches per call."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmoe_amd import hip                                                 # noqa: E402
from pmoe_amd.augment import get_augmenter                               # noqa: E402
from pmoe_amd.preprocess import FramePreprocessor                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs the MI355X (no CPU path, no CPU timing)")
    torch.manual_seed(0)
    frames = torch.randint(0, 256, (a.frames, 600, 800, 3), dtype=torch.uint8, device="cuda")
    pre = FramePreprocessor(crop=(125, 90), size=(a.size, a.size))
    variants = [("a: pre(frames)", None),
                ("b: + super_hard @ 64000", get_augmenter(64000, 64, "super_hard")),
                ("c: + segmentation", get_augmenter(aug_type="segmentation"))]
    gen = torch.Generator().manual_seed(1)

    def call(aug):
        return pre(frames) if aug is None else pre(frames, augment=aug, generator=gen)

    launches = {}
    for name, aug in variants:
        for _ in range(a.warmup):
            call(aug)
        with hip.LaunchRecorder() as rec:
            call(aug)
        launches[name] = len(rec.calls)
    torch.cuda.synchronize()
    wall = {name: [] for name, _ in variants}
    devt = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, aug in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.calls):
                call(aug)
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
            devt[name].append(e0.elapsed_time(e1) / a.calls)
    print(f"{a.frames} frames 600 x 800 -> {a.size} x {a.size}; {a.calls} calls per window, {a.rounds} rounds (median [min .. max])")
    for name, aug in variants:
        w, d = wall[name], devt[name]
        line = (f"  {name:26s} wall {statistics.median(w):7.3f} ms [{min(w):.3f} .. {max(w):.3f}]   "
                f"device {statistics.median(d):7.3f} ms [{min(d):.3f} .. {max(d):.3f}]   {launches[name]} launches (last warm call)")
        if aug is not None:
            t0 = time.perf_counter()
            for _ in range(a.calls):
                plan = aug.plan(a.frames, a.size, a.size, generator=gen)
            host = (time.perf_counter() - t0) * 1e3 / a.calls
            line += f"   host plan {host:.3f} ms ({float(plan.n_slots.double().mean()):.2f} ops / frame)"
        print(line)
    base = statistics.median(wall[variants[0][0]])
    for name, _ in variants[1:]:
        print(f"  {name.split(':')[0]} - a = {statistics.median(wall[name]) - base:.3f} ms wall per {a.frames} frames")


if __name__ == "__main__":
    main()
