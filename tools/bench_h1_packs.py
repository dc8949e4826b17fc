#!/usr/bin/env python3
"""The full H1 training step (bench.py: forward, moe_loss, backward, clip_grad_norm_(1.0) fused into FusedAdam(amsgrad)) at the
headline shape, with and without ``FusedAdam(packs=model)`` -- does the optimizer writing the engine's packed weights pay for
itself against the per-layer repack it saves?
  python tools/bench_h1_packs.py [--batch 64] [--size 256] [--experts 4] [--dtype bf16] [--steps 10] [--warmup 3] [--rounds 5]
         [--optimizer adam|rmsprop] [--lr LR] [--out profiles/h1_packs.json]
Two identical models (one per leg) in one process; the legs alternate round by round, every step is timed with device events.
Reports, per leg, the median ms/step of every round, their median and spread over the rounds, and the number of pack launches
(ops.pack_conv_weights + ops.pack_bias calls) per step.

``--optimizer rmsprop``: the trainers' other optimizer (``conf/stage_2*.yaml`` ``rmsprop:``, centered) -- FusedRMSprop in the two
legs, and a third leg ``torch``: what a user of ``optimizer: rmsprop`` had before, torch.nn.utils.clip_grad_norm_ +
torch.optim.RMSprop(centered=True) on the same model.  Its learning rate defaults to 2e-5, a tenth of the shipped block's, as a
precaution: the first centred update moves EVERY weight by 10 lr, and at 2e-4 a two-image test model was once seen to come back
with standard deviations of 0 after one step (tests/test_rmsprop_gpu.py); this tool was not run at 2e-4.  The time of
a step does not depend on it."""
import argparse
import copy
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from pmoe_amd import ops, optim                                         # noqa: E402
from pmoe_amd.loss import moe_loss                                      # noqa: E402
from pmoe_amd.model.moe import get_model                                # noqa: E402
from pmoe_amd.utils import stage2_model_cfg                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--experts", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--steps", type=int, default=10, help="timed steps per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--optimizer", default="adam", choices=["adam", "rmsprop"])
    ap.add_argument("--lr", type=float, default=None, help="default: 2e-4 (adam), 2e-5 (rmsprop)")
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    base = get_model(stage2_model_cfg("moe", a.experts, dropout=0.0)).to(dev)
    base.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    base.train()
    g = torch.Generator().manual_seed(1234)
    B = a.batch
    images = torch.rand(B, 4, 3, a.size, a.size, generator=g).to(dev)
    speed = torch.rand(B, 1, generator=g).to(dev)
    target = torch.rand(B, 1, generator=g).to(dev)
    command = torch.nn.functional.one_hot(torch.randint(0, 6, (B,), generator=g), 6).float().to(dev)
    control = (torch.rand(B, 2, generator=g) * 2 - 1).to(dev)

    calls = [0]
    for name in ("pack_conv_weights", "pack_bias"):
        def counted(*args, _fn=getattr(ops, name), **kw):
            calls[0] += 1
            return _fn(*args, **kw)
        setattr(ops, name, counted)

    rms = a.optimizer == "rmsprop"
    lr = a.lr if a.lr is not None else (2e-5 if rms else 2e-4)
    rms_block = dict(lr=lr, momentum=0, alpha=0.99, eps=1e-8, centered=True, weight_decay=0)
    legs = {}
    for leg in ("plain", "packs") + (("torch",) if rms else ()):
        model = copy.deepcopy(base)
        packs = model if leg == "packs" else None
        if leg == "torch":
            opt = torch.optim.RMSprop(model.parameters(), **rms_block)
        elif rms:
            opt = optim.FusedRMSprop(model.parameters(), **rms_block, packs=packs)
        else:
            opt = optim.FusedAdam(model.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=True, packs=packs)
        legs[leg] = (model, opt)

    def step(leg):
        model, opt = legs[leg]
        d, s = model(images, speed, command)
        loss = moe_loss(d, s, control, target, [0.7, 0.3])
        opt.zero_grad()
        loss.backward()
        if leg == "torch":
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            return
        gn = optim.clip_grad_norm_(model.parameters(), 1.0, scale=False)
        opt.step(clip=gn)

    out = {"shape": f"E={a.experts} B={a.batch} {a.size}x{a.size} {a.dtype}", "steps_per_round": a.steps, "rounds": a.rounds,
           "step": "fwd+moe_loss+bwd+clip_grad_norm_(1.0)+" + (f"FusedRMSprop(centered, lr {lr:g}); leg torch: torch's clip_grad_norm_"
                                                              " + RMSprop(centered)" if rms else "FusedAdam(amsgrad)"), "legs": {}}
    for leg in legs:
        for _ in range(a.warmup):
            step(leg)
        calls[0] = 0
        step(leg)
        out["legs"][leg] = {"pack_launches_per_step": calls[0], "round_ms": []}
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for leg in legs:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            ev[0].record()
            for i in range(a.steps):
                step(leg)
                ev[i + 1].record()
            torch.cuda.synchronize()
            out["legs"][leg]["round_ms"].append(round(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)), 3))
    for leg, r in out["legs"].items():
        r["ms_per_step"] = round(statistics.median(r["round_ms"]), 3)
        r["round_spread_ms"] = round(max(r["round_ms"]) - min(r["round_ms"]), 3)
        print(f"H1 step, {leg:5s}: {r['ms_per_step']:.3f} ms/step (median of {a.rounds} rounds x {a.steps} steps; rounds "
              f"{r['round_ms']}), {r['pack_launches_per_step']} pack launches per step")
    out["gain_ms"] = round(out["legs"]["plain"]["ms_per_step"] - out["legs"]["packs"]["ms_per_step"], 3)
    print(f"plain - packs = {out['gain_ms']:.3f} ms/step; round-to-round spread "
          f"{max(r['round_spread_ms'] for r in out['legs'].values()):.3f} ms")
    if rms:
        out["torch_minus_plain_ms"] = round(out["legs"]["torch"]["ms_per_step"] - out["legs"]["plain"]["ms_per_step"], 3)
        print(f"torch - plain = {out['torch_minus_plain_ms']:.3f} ms/step")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
