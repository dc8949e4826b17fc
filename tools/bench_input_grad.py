#!/usr/bin/env python3
"""The gradient with respect to the images at the headline shape (E = 4 experts, B = 64, 256 x 256, bf16).
  python tools/bench_input_grad.py [--experts 4] [--batch 64] [--size 256] [--calls 10] [--steps 3] [--rounds 5] [--warmup 2]
Times, with device events, the legs of each pair alternating inside every round, the median over `rounds` rounds:
  (a) pmoe_stem_input_grad alone: dz1 [E*B,H,W,64] -> f32 [B,12,H,W], experts summed inside the reduction
  (b) the same gradient from entry points that were there before it: the per-(expert, image) data-gradient convolution with the
      gated pack and the dgap bias into bf16 NHWC [E*B,H,W,16], a torch sum over the experts, nhwc_to_nchw
  (c) a training step (forward, moe_loss, backward) of the mixture without and with images.requires_grad
and prints for (a) the bytes the algorithm needs (dz1 read once + the planes written) over its time."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmoe_amd import hip, ops                                            # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(legs, calls, rounds, warmup):
    for _, fn in legs:
        for _ in range(warmup):
            fn()
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            times[name].append(timed(fn, calls))
    return times


def show(name, t, extra=""):
    print(f"  {name:44s} {statistics.median(t):8.3f} ms [{min(t):.3f} .. {max(t):.3f}]{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad: needs the MI355X (no CPU path, no CPU timing)")
    E, B, H, C = a.experts, a.batch, a.size, 12
    N, dev = E * B, "cuda"
    torch.manual_seed(0)
    print(f"E={E} B={B} {H} x {H} bf16; {a.calls} calls ({a.steps} steps) per window, {a.rounds} rounds (median [min .. max])")

    # ---- (a) / (b): the launch and its assembled equivalent on the same operands
    dz1 = torch.randn(N, H, H, 64, device=dev, dtype=BF16)
    ws = [torch.randn(64, C, 3, 3, device=dev) / 8 for _ in range(E)]
    gate = torch.rand(N, 16, device=dev)
    dgap = torch.randn(N, 16, device=dev) / 4
    wd = torch.empty(N, 64, 9, 64, dtype=BF16, device=dev)
    ops.pack_conv_weights_gated(hip.ptr_table(ws, dev), gate, None, wd, N, B, 64, C, 3, 64, 16, 64, 64, BF16)
    dx_a = torch.empty(B, C, H, H, dtype=F32, device=dev)
    dx_b = torch.empty(B, C, H, H, dtype=F32, device=dev)
    g = torch.empty(N, H, H, 16, dtype=BF16, device=dev)
    bias_b = torch.zeros(N, 64, device=dev)            # (the conv's bias rows are coutp = 64 wide)
    bias_b[:, :16] = dgap

    def leg_a():
        ops.stem_input_grad(dz1, wd, dgap, dx_a, E)

    def leg_b():
        ops.conv2d(dz1, wd, g, bias=bias_b, cin=64, cout=16, coutp=64, ipe=1, ks=3, stride=1, pad=1, dilate=False, in_coff=0,
                   out_coff=0)
        ops.nhwc_to_nchw(g.view(E, B, H, H, 16).sum(0, dtype=F32), dx_b, C)

    t = alternate([("a", leg_a), ("b", leg_b)], a.calls, a.rounds, a.warmup)
    nbytes = dz1.numel() * 2 + dx_a.numel() * 4
    show("(a) stem_input_grad", t["a"], f"   {nbytes / 1e9:.3f} GB needed -> {nbytes / statistics.median(t['a']) / 1e9:.2f} TB/s")
    show("(b) conv2d dgrad + sum over experts + nhwc_to_nchw", t["b"])
    print(f"  (a) < (b) in {sum(x < y for x, y in zip(t['a'], t['b']))} of {a.rounds} paired rounds; "
          f"(a) vs (b) rel-L2 {((dx_a - dx_b).norm() / dx_b.norm()).item():.2e} (b rounds every expert's term to bf16)")
    del dz1, g, wd, dx_a, dx_b
    torch.cuda.empty_cache()

    # ---- (c): the training step without and with the image gradient
    from pmoe_amd.loss import moe_loss
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    model = get_model(stage2_model_cfg("moe", E, dropout=0.0)).to(dev)
    model.compute_dtype = BF16
    model.train()
    command = torch.zeros(B, 6, device=dev)
    command[torch.arange(B), torch.randint(0, 6, (B,))] = 1.0
    inp = dict(images=torch.rand(B, 4, 3, H, H, device=dev), speed=torch.rand(B, 1, device=dev), command=command,
               control=torch.rand(B, 2, device=dev) * 2 - 1, target_speed=torch.rand(B, 1, device=dev))
    img_leaf = inp["images"].clone().requires_grad_(True)

    def step(images):
        model.zero_grad(set_to_none=True)
        dist, speeds = model(images, inp["speed"], inp["command"])
        moe_loss(dist, speeds, inp["control"], inp["target_speed"], [0.7, 0.3]).backward()

    t = alternate([("without", lambda: step(inp["images"])), ("with", lambda: step(img_leaf))], a.steps, a.rounds, a.warmup)
    show("(c) training step", t["without"])
    show("(c) training step, images.requires_grad", t["with"])
    print(f"  (c) with - without = {statistics.median(t['with']) - statistics.median(t['without']):.3f} ms per step")
    ops.profile_begin()
    step(img_leaf)
    rec = [(n, m, ms) for n, m, ms in ops.profile_end() if n in ("stem_input_grad", "pack_conv_weights_gated") or
           str(m.get("name", "")).startswith("stem.bn1")]
    for n, m, ms in rec:
        print(f"    in that step: {n:26s} {m.get('name', ''):18s} {ms:7.3f} ms")


if __name__ == "__main__":
    main()
