#!/usr/bin/env python3
"""Stage-0 U-Net training step (trainer/train_0.py:130-140, conf/stage_0.yaml: batch 64 at 224 x 224): UNet.forward,
cross_entropy_tversky_weighted_loss, backward -- and the same with the FusedAdam(amsgrad) step.
  python tools/bench_stage0.py [--batch 64] [--size 224] [--steps 5] [--dtype bf16] [--dropout 0.0] [--profile]
Reports ms/step, launches per step, the per-kernel table (--profile) and algorithmic TFLOP/s: forward + data gradient + weight
gradient of every layer (3 x 2 x GMAC x batch) less the data gradient of the first convolution, whose input is the image."""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmoe_amd import ops                                                # noqa: E402
from pmoe_amd.loss import cross_entropy_tversky_weighted_loss, dice_score   # noqa: E402
from pmoe_amd.model import blocks as B                                  # noqa: E402
from pmoe_amd.optim import FusedAdam                                    # noqa: E402
from tools.bench_stage1 import unet_gmac                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    model = B.UNet(dropout=a.dropout).to(dev)
    model.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-3, amsgrad=True)
    image = torch.rand(a.batch, 3, a.size, a.size, device=dev)
    target = torch.randint(0, 23, (a.batch, a.size, a.size), device=dev)

    def step(with_opt):
        out = model(image)
        loss = cross_entropy_tversky_weighted_loss(out, target)
        opt.zero_grad()
        loss.backward()
        if with_opt:
            opt.step()
        return loss, out

    gmac = unet_gmac(a.size, a.size)
    first_dgrad = a.size * a.size * 9 * 3 * 64 / 1e9
    gflop = 2 * (3 * gmac - first_dgrad)
    print(f"U-Net forward {gmac:.3f} GMAC/sample; step {a.batch * gflop / 1e3:.2f} TFLOP (algorithmic)")
    for with_opt, what in ((False, "forward + loss + backward"), (True, "forward + loss + backward + FusedAdam(amsgrad)")):
        for _ in range(a.warmup):
            step(with_opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss, out = step(with_opt)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        print(f"UNet stage-0 {what} B={a.batch} {a.size}x{a.size} {a.dtype} dropout={a.dropout}: {ms:.1f} ms/step = "
              f"{a.batch / ms * 1e3:.1f} samples/s, {a.batch * gflop / ms:.0f} TFLOP/s algorithmic, loss {loss.item():.4f}")
    print(f"peak memory GiB: {torch.cuda.max_memory_allocated() / 2**30:.2f}")
    logits = out.detach()
    for _ in range(3):
        d = dice_score(logits, target)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        d = dice_score(logits, target)
    torch.cuda.synchronize()
    mb = logits.numel() * 4 / 1e6
    ms = (time.perf_counter() - t0) / 10 * 1e3
    print(f"dice_score on the step's logits ({mb:.0f} MB, warm, mean of 10 calls): {ms:.3f} ms = {mb / ms:.0f} GB/s, "
          f"mean dice {d.mean().item():.4f}")
    ops.profile_begin()
    step(True)
    rows = ops.profile_end()
    print(f"launches per step (forward + loss + backward, library calls; the optimizer's are its own): {len(rows)}")
    if a.profile:
        agg = {}
        for name, meta, ms_ in rows:
            e = agg.setdefault(name, [0.0, 0])
            e[0] += ms_
            e[1] += 1
        total = sum(v[0] for v in agg.values())
        print(f"per-kernel table (event-timed one by one: sum {total:.1f} ms)")
        for k, (ms_, n) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:24]:
            print(f"  {k:24s} {ms_:8.2f} ms {n:5d} launches")
        layers = {}
        for name, meta, ms_ in rows:
            if name in ("conv2d", "conv2d_wgrad") and "name" in meta:
                e = layers.setdefault((name, meta["name"]), [0.0, 0, 0.0])
                e[0] += ms_
                e[1] += 1
                e[2] += meta.get("flop", 0.0)
        for (op, nm), (ms_, n, fl) in sorted(layers.items(), key=lambda kv: -kv[1][0])[:30]:
            print(f"  {op:13s} {nm:28s} {ms_:7.2f} ms {n:4d} launches {fl / ms_ / 1e9:7.0f} TFLOP/s")


if __name__ == "__main__":
    main()
