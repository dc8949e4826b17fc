#!/usr/bin/env python3
"""One step of the closed-loop agent (autoagents/image_agent.py:114-177) at its real shape -- a 600x800 BGRA camera frame, a speed
and a RoadOption value in, (steer, throttle, brake) out, B=1, 224x224, the model of tools/bench_infer.py -- two ways, alternating in
one process:

  (a) the path a caller assembled around ``PolicyTick`` before ``AgentStep`` existed: host flip + copy, upload,
      ``FramePreprocessor``, the speed and one-hot command tensors of the reference, ``PolicyTick(mode="plan")``, ``.cpu()``, the
      reference's ``postprocess`` with its ``.item()`` reads;
  (b) ``AgentStep(mode="plan").step(bgra, spd, cmd)``.

Host wall clock per step (each leg ends in a synchronisation): warm-up, then 5 rounds of 200 steps per leg, per round the median,
minimum and maximum; then the device-event time of (b)'s launches alone.  ``--model moe|punet|pmoe`` (default moe; the expert count
is the first argument, default 3).  The last line is the same as JSON."""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS, STEPS, WARMUP = 5, 200, 30
SENSOR, CROP, SIZE = (600, 800), (125, 90), (224, 224)


def build_model(kind, experts):
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import build_product, stage2_model_cfg
    if kind == "moe":
        return get_model(stage2_model_cfg("moe", experts, dropout=0.3)).cuda().eval()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:               # random-init checkpoint files: the constructors read them
        return build_product(Path(tmp), dict(type=kind, n_experts=experts, future_frames=6)).cuda().eval()


class ParentPath:
    def __init__(self, model, seed):
        from pmoe_amd.infer import PolicyTick
        from pmoe_amd.preprocess import FramePreprocessor
        self.transform = FramePreprocessor(crop=CROP, size=SIZE)
        self.tick = PolicyTick(model, batch=1, height=SIZE[0], width=SIZE[1], mode="plan", seed=seed)
        self.n_commands = self.tick.static_in[2].shape[1]

    @staticmethod
    def postprocess(action):
        """image_agent.py:114-125 with a tuple in place of carla.VehicleControl"""
        steer = torch.clip(action[0], -1.0, 1.0).item()
        if action[1] < -0.5:
            throttle = 0
            brake = torch.clip(-action[1], 0.0, 1.0).item()
            steer = 0
        else:
            throttle = max(torch.clip(action[1], 0.0, 0.75).item(), 0.4)
            brake = 0
        return steer, throttle, brake

    def step(self, bgra, spd, cmd):
        rgb = bgra[..., :3].copy()
        rgb = rgb[..., ::-1]                                  # BGR -> RGB
        rgb = self.transform(torch.from_numpy(rgb.copy()).cuda())
        cmd_value = cmd - 1
        cmd_value = 3 if cmd_value < 0 else cmd_value
        speed = torch.tensor([spd / 10.0, ], dtype=torch.float).unsqueeze_(0).cuda()
        command = torch.zeros(self.n_commands).scatter_(dim=0, index=torch.tensor(int(cmd_value)), value=1).unsqueeze_(0).cuda()
        action = self.tick(rgb.unsqueeze(0), speed, command).squeeze().cpu()
        return self.postprocess(action)


def main():
    kind = sys.argv[sys.argv.index("--model") + 1] if "--model" in sys.argv else "moe"
    if kind not in ("moe", "punet", "pmoe"):
        raise SystemExit("--model moe|punet|pmoe")
    experts = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 3
    from pmoe_amd.infer import AgentStep
    model = build_model(kind, experts)
    parent = ParentPath(model, seed=0)
    agent = AgentStep(model, sensor=SENSOR, crop=CROP, size=SIZE, batch=1, mode="plan", seed=0)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, SENSOR + (4,), dtype=np.uint8) for _ in range(8)]
    inputs = [(frames[i % 8], float(rng.uniform(0.0, 9.0)), [-1, 1, 2, 3, 4][i % 5]) for i in range(STEPS)]

    legs = {"a": parent.step, "b": agent.step}
    for i in range(WARMUP):                                   # the same inputs, the same seed: the same control
        bgra, spd, cmd = inputs[i]
        a, b = legs["a"](bgra, spd, cmd), legs["b"](bgra, spd, cmd)[0]
        assert tuple(float(v) for v in a) == tuple(b.tolist()), (i, a, b)
    rounds = {"a": [], "b": []}
    for r in range(ROUNDS):
        for name in (("a", "b") if r % 2 == 0 else ("b", "a")):
            step, times = legs[name], []
            torch.cuda.synchronize()
            for bgra, spd, cmd in inputs:
                t0 = time.perf_counter()
                step(bgra, spd, cmd)
                times.append((time.perf_counter() - t0) * 1e3)
            rounds[name].append(times)
    label = kind if kind == "punet" else f"{kind} E={experts}"
    print(f"{label}  600x800 BGRA -> 224x224, B=1, plan mode; host wall clock per step, ms: median (min .. max) of {STEPS} steps per round")
    for r in range(ROUNDS):
        a, b = rounds["a"][r], rounds["b"][r]
        print(f"  round {r + 1}: (a) parent path {statistics.median(a):.3f} ({min(a):.3f} .. {max(a):.3f})   "
              f"(b) AgentStep {statistics.median(b):.3f} ({min(b):.3f} .. {max(b):.3f})   (a) / (b) = "
              f"{statistics.median(a) / statistics.median(b):.2f}")
    med = {k: statistics.median(statistics.median(t) for t in v) for k, v in rounds.items()}
    every = all(statistics.median(b) < statistics.median(a) for a, b in zip(rounds["a"], rounds["b"]))

    # device time of (b)'s launches alone: events around the plan, after the uploads were queued
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    device_ms = []
    for bgra, spd, cmd in inputs:
        agent.step(bgra, spd, cmd)                            # (fills the pinned buffers; the plan below runs on the same bytes)
        e0.record()
        agent.tick._issue()
        e1.record()
        e1.synchronize()
        device_ms.append(e0.elapsed_time(e1))
    calls = len(agent.tick.plan.calls)

    # the first launch against the three it replaces, 200 back to back between two events
    from pmoe_amd import ops
    dev_rgb = torch.from_numpy(np.ascontiguousarray(frames[0][..., 2::-1])).cuda()

    def per_call(fn):
        fn()
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / STEPS
    push_ms = per_call(agent.tick._push)
    chain_ms = per_call(lambda: ops.history_push(parent.tick.frames, parent.transform(dev_rgb).unsqueeze(0), nhwc=parent.tick.newest))
    print(f"  median of the round medians: (a) {med['a']:.3f} ms  (b) {med['b']:.3f} ms  ({med['a'] / med['b']:.2f}x); "
          f"(b) < (a) in every paired round: {every}")
    print(f"  (b) device-event time of its {calls} recorded launches (sensor push .. control): median {statistics.median(device_ms):.3f} ms "
          f"({min(device_ms):.3f} .. {max(device_ms):.3f}); PolicyTick's plan: {len(parent.tick.plan.calls)} launches")
    print(f"  pmoe_sensor_push {push_ms * 1e3:.1f} us per call; horizontal + vertical pass + pmoe_history_push {chain_ms * 1e3:.1f} us "
          f"({STEPS} calls back to back between two events)")
    print(json.dumps({"model": label, "steps_per_round": STEPS, "rounds": ROUNDS,
                      "parent_ms": [round(statistics.median(t), 4) for t in rounds["a"]],
                      "agent_ms": [round(statistics.median(t), 4) for t in rounds["b"]],
                      "parent_median_ms": round(med["a"], 4), "agent_median_ms": round(med["b"], 4),
                      "agent_faster_every_round": every, "agent_device_ms": round(statistics.median(device_ms), 4),
                      "agent_launches": calls, "sensor_push_us": round(push_ms * 1e3, 2),
                      "replaced_chain_us": round(chain_ms * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
