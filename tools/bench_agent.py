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
is the first argument, default 3).  The last line is the same as JSON.

``--log``: the cost of the video log instead (``main_log``): ``AgentStep`` without a log, with a ``pmoe_amd.vision.FrameLog``, and
without one plus the newest frame brought to the host and normalised with numpy; then the device time of one
``pmoe_frame_annotate`` launch."""
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


def main_log(kind, experts):
    """``--log``: what the reference's video log (``image_agent.py:167-173``) costs per step, three legs alternating in one
    process: (a) ``AgentStep`` without a log; (b) with a ``FrameLog``; (c) without a log plus what a caller does without one:
    the newest frame of the ring to the host and the reference's numpy normalisation (no text)."""
    from pmoe_amd import vision
    from pmoe_amd.infer import AgentStep
    model = build_model(kind, experts)
    plain = AgentStep(model, sensor=SENSOR, crop=CROP, size=SIZE, batch=1, mode="plan", seed=0)
    log = vision.FrameLog(capacity=1000, size=SIZE, device="cuda")
    logged = AgentStep(model, sensor=SENSOR, crop=CROP, size=SIZE, batch=1, mode="plan", seed=0, log=log)
    hosted = AgentStep(model, sensor=SENSOR, crop=CROP, size=SIZE, batch=1, mode="plan", seed=0)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, SENSOR + (4,), dtype=np.uint8) for _ in range(8)]
    inputs = [(frames[i % 8], float(rng.uniform(0.0, 9.0)), [-1, 1, 2, 3, 4][i % 5]) for i in range(STEPS)]
    vizs = []

    def host_log(bgra, spd, cmd):
        control = hosted.step(bgra, spd, cmd)
        img = hosted.tick.frames[:, -1].cpu()[0].permute(1, 2, 0).numpy()
        vizs.append((((img - img.min()) / (-img.min() + img.max())) * 255).astype(np.uint8))
        if len(vizs) > 1000:
            vizs.clear()
        return control

    legs = {"a": plain.step, "b": logged.step, "c": host_log}
    for i in range(WARMUP):
        bgra, spd, cmd = inputs[i]
        a, b, c = (legs[k](bgra, spd, cmd) for k in "abc")
        assert np.array_equal(a, b) and np.array_equal(a, c), (i, a, b, c)
    assert np.array_equal(log.frames()[-1][100:], vizs[-1][100:])            # (below the text rows: the same pixels)
    rounds = {k: [] for k in legs}
    for r in range(ROUNDS):
        for name in ("abc"[r % 3:] + "abc"[:r % 3]):
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
        print(f"  round {r + 1}: " + "   ".join(
            f"({k}) {what} {statistics.median(rounds[k][r]):.3f} ({min(rounds[k][r]):.3f} .. {max(rounds[k][r]):.3f})"
            for k, what in (("a", "no log"), ("b", "FrameLog"), ("c", "frame to host + numpy"))))
    med = {k: statistics.median(statistics.median(t) for t in v) for k, v in rounds.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tick = logged.tick

    def push():
        log.push(tick.frames[:, -1], tick.raw if tick.pun is None else tick._result[0], tick.static_in[1], tick.static_in[2])
    from pmoe_amd import hip
    push()
    with hip.LaunchRecorder() as one:                         # the launch alone, re-issued without the Python above it
        push()
    assert [c[0].__name__ for c in one.calls] == ["pmoe_frame_annotate"]
    e0.record()
    for _ in range(STEPS):
        one.replay()
    e1.record()
    e1.synchronize()
    annotate_us = e0.elapsed_time(e1) / STEPS * 1e3
    print(f"  median of the round medians: (a) {med['a']:.3f} ms  (b) {med['b']:.3f} ms  (c) {med['c']:.3f} ms;  "
          f"(b) - (a) = {(med['b'] - med['a']) * 1e3:.1f} us,  (c) - (a) = {(med['c'] - med['a']) * 1e3:.1f} us")
    print(f"  pmoe_frame_annotate {annotate_us:.1f} us per launch ({STEPS} launches back to back between two events); "
          f"the log holds {len(log)} frames, {log.dropped} overwritten")
    print(json.dumps({"model": label, "steps_per_round": STEPS, "rounds": ROUNDS,
                      **{f"{k}_ms": [round(statistics.median(t), 4) for t in v] for k, v in rounds.items()},
                      **{f"{k}_median_ms": round(v, 4) for k, v in med.items()}, "frame_annotate_us": round(annotate_us, 2)}), flush=True)


def main():
    kind = sys.argv[sys.argv.index("--model") + 1] if "--model" in sys.argv else "moe"
    if kind not in ("moe", "punet", "pmoe"):
        raise SystemExit("--model moe|punet|pmoe")
    experts = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 3
    if "--log" in sys.argv:
        return main_log(kind, experts)
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
