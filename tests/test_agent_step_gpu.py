"""pmoe_amd.infer.AgentStep on the GPU: pmoe_sensor_push against the launches it replaces (horizontal pass, vertical pass, history
push) and the Pillow fixtures, pmoe_control_postprocess against its numpy statement, and a whole step -- BGRA bytes, speed and
RoadOption value in, control out -- against the path a caller had to assemble before: host flip, upload, FramePreprocessor,
PolicyTick, download, postprocess.  Every comparison is exact."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.make_prep_golden import CASES, frame
from tests import agent_ref

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
_BY_NAME = {c[0]: c for c in CASES}

# name (of oracle/make_prep_golden.CASES, or the sizes themselves), B, T, NHWC (dtype, Cp) or None
PUSH_CASES = [
    ("agent_600x800_to_224", 1, 4, (torch.bfloat16, 16)),              # the agent's shape
    ("odd_301x203_to_97x65", 2, 1, None),                               # tail tile, odd width, T = 1 has no shift
    ("upsample_100x90_to_224x160", 2, 3, (torch.float32, 4)),           # scale < 1: tiles share source rows
    ("small_240x320_to_128", 3, 4, (torch.bfloat16, 8)),
    ((400, 48, (0, 0), (8, 64)), 1, 2, None),                           # the reduced tile: 8 rows would need 76 800 bytes
]


def _tables(w0, w, rows, h, dev="cuda"):
    from pmoe_amd.preprocess import _coeffs
    out = []
    for k, b, c in (_coeffs(w0, w), _coeffs(rows, h)):
        out.append((k, torch.tensor(b, dtype=torch.int32, device=dev), torch.tensor(c, dtype=torch.int32, device=dev)))
    return out[0], out[1], out[1][1].tolist()


@pytest.mark.parametrize("case", PUSH_CASES, ids=[c[0] if isinstance(c[0], str) else "reduced_tile_400x48_to_8x64" for c in PUSH_CASES])
def test_sensor_push_equals_the_chain_it_replaces(case):
    """two pushes into a ring prefilled with random f32 -- a frame whose B, G, R differ at every pixel, then the fixture's frame
    (item 0 of the batch) -- against ops.history_push(ring, FramePreprocessor(crop, size)(rgb), nhwc) on a copy: ring and NHWC
    tensor equal after each, the newest slot equal to Pillow's output / 255, the source bytes untouched"""
    from pmoe_amd import ops
    from pmoe_amd.preprocess import FramePreprocessor
    spec, B, T, nhwc_spec = case
    if isinstance(spec, str):
        _, H0, W0, crop, size, seed = _BY_NAME[spec]
        fixture = np.load(GOLDEN / "prep.npz")[spec]
    else:
        (H0, W0, crop, size), seed, fixture = spec, 31, None
    h, w = size
    rows = H0 - crop[0] - crop[1]
    htable, vtable, vbounds = _tables(W0, w, rows, h)
    tile = ops.sensor_tile(vbounds, w)
    assert tile[0] == (8 if isinstance(spec, str) else 4)
    gen = torch.Generator().manual_seed(seed)
    ring = torch.rand(B, T, 3, h, w, generator=gen).cuda()
    ref_ring = ring.clone()
    nhwc = ref_nhwc = None
    if nhwc_spec is not None:
        nhwc = torch.full((B, h, w, nhwc_spec[1]), 7.0, dtype=nhwc_spec[0], device="cuda")
        ref_nhwc = nhwc.clone()
    pre = FramePreprocessor(crop, size)
    first = frame(H0, W0, seed)
    pushes = [agent_ref.distinct_rgb((B, H0, W0), seed + 100),
              np.stack([first] + [np.ascontiguousarray(np.flip(first, b % 2)) for b in range(1, B)])]
    for n, rgb in enumerate(pushes):
        bgra = agent_ref.bgra_of(rgb, seed + n)
        assert (bgra[..., 0] != bgra[..., 2]).any() and bgra[..., 3].std() > 50.0
        if n == 0:
            assert (bgra[..., 0] != bgra[..., 1]).all() and (bgra[..., 1] != bgra[..., 2]).all() and (bgra[..., 0] != bgra[..., 2]).all()
        dev_bgra = torch.from_numpy(bgra).cuda()
        ops.sensor_push(dev_bgra, ring, crop[0], rows, htable, vtable, tile, nhwc=nhwc)
        item = pre(torch.from_numpy(rgb).cuda())
        ops.history_push(ref_ring, item, nhwc=ref_nhwc)
        assert torch.equal(ring, ref_ring), (n, (ring - ref_ring).abs().max().item())
        if nhwc is not None:
            assert torch.equal(nhwc, ref_nhwc), n
        assert torch.equal(dev_bgra.cpu(), torch.from_numpy(bgra)), "the launch wrote into its source"
    if fixture is not None:
        want = torch.from_numpy(fixture.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
        assert torch.equal(ring[0, T - 1].cpu(), want)


def test_sensor_push_refuses_what_does_not_fit():
    from pmoe_amd import ops
    h, w, rows = 8, 224, 1200
    htable, vtable, vbounds = _tables(64, w, rows, h)
    tile = ops.sensor_tile(vbounds, w)
    assert tile == (1, 300)
    bgra = torch.zeros(1, rows, 64, 4, dtype=torch.uint8, device="cuda")
    ring = torch.ones(1, 2, 3, h, w, device="cuda")
    with pytest.raises(NotImplementedError, match="1200"):
        ops.sensor_push(bgra, ring, 0, rows, htable, vtable, tile)
    assert bool((ring == 1).all())
    with pytest.raises(ValueError, match="sensor_push"):
        ops.sensor_push(bgra[..., :3].contiguous(), ring, 0, rows, htable, vtable, tile)


def _edge_values():
    vals = []
    for v in (-1.0, -0.5, 0.0, 0.4, 0.75, 1.0):
        v = np.float32(v)
        vals += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    vals += [np.float32(x) for x in (-0.0, 0.3, 0.6, 2.0, -3.0, -7.0, 0.1, 0.9, 0.2, 0.5, np.inf, -np.inf, np.nan, 1e-40, -1e-40)]
    return np.array(vals, dtype=np.float32)


def test_control_kernel_against_its_statement():
    """every pair of: -1, -0.5, 0, 0.4, 0.75, 1 and their f32 neighbours on both sides, the values of the rule's table, -0.0, two
    subnormals, the infinities and NaN -- bits and NaN positions"""
    from pmoe_amd import ops
    v = _edge_values()
    actions = np.stack(np.meshgrid(v, v, indexing="ij"), -1).reshape(-1, 2)
    assert actions.shape[0] == v.size ** 2 > 1000                      # several workgroups
    control = torch.full((actions.shape[0], 3), -9.0, dtype=torch.float64, device="cuda")
    ops.control_postprocess(torch.from_numpy(actions).cuda(), control)
    got, want = control.cpu().numpy(), agent_ref.control_ref(actions)
    bad = [(a.tolist(), g.tolist(), r.tolist()) for a, g, r in zip(actions, got, want) if not agent_ref.same_bits(g, r)]
    assert not bad, bad[:5]
    table = np.array([a for a, _ in agent_ref.CONTROL_TABLE], dtype=np.float32)
    out = torch.zeros(len(table), 3, dtype=torch.float64, device="cuda")
    ops.control_postprocess(torch.from_numpy(table).cuda(), out)
    assert agent_ref.same_bits(out.cpu().numpy(), np.array([w for _, w in agent_ref.CONTROL_TABLE]))
    with pytest.raises(ValueError, match="control_postprocess"):
        ops.control_postprocess(torch.zeros(2, 2, device="cuda"), torch.zeros(2, 2, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------ a whole step
class _ParentPath:
    """what a caller assembled around PolicyTick before AgentStep (image_agent.py:132-160): host flip and
    copy, upload, FramePreprocessor, speed and one-hot command tensors, the tick, download, the postprocess rule"""

    def __init__(self, model, B, crop, size, mode, seed, n_commands):
        from pmoe_amd.infer import PolicyTick
        from pmoe_amd.preprocess import FramePreprocessor
        self.pre = FramePreprocessor(crop, size)
        self.tick = PolicyTick(model, batch=B, height=size[0], width=size[1], mode=mode, seed=seed)
        self.n_commands = n_commands

    def step(self, bgra, spds, cmds):
        rgb = bgra[..., :3].copy()[..., ::-1]
        frame_ = self.pre(torch.from_numpy(rgb.copy()).cuda())
        speed = torch.tensor([[s / 10.0] for s in spds], dtype=torch.float).cuda()
        command = torch.from_numpy(agent_ref.onehot_ref(cmds, self.n_commands)).cuda()
        actions = self.tick(frame_, speed, command).cpu()
        return agent_ref.control_ref(actions.numpy())


def _frames(B, H0, W0, seed):
    rng = np.random.default_rng(seed)
    while True:
        yield agent_ref.bgra_of(rng.integers(0, 256, (B, H0, W0, 3), dtype=np.uint8), int(rng.integers(1 << 30)))


def _model(tmp_path, name):
    from tests.test_policy_tick_gpu import _moe_model, _punet_model
    if name.startswith("g"):
        return _moe_model(name, torch.bfloat16)
    exclude = ["lat_weights", "long_weights"] if "pmoe" in name else ()
    return _punet_model(tmp_path, name, torch.bfloat16, exclude_freeze=exclude)


@pytest.mark.parametrize("name", ["g4_moealt_e4_b2_64", "p3_punetinter_b2_64_f2", "p5_pmoe_e2_b2_64_f2", "g2_moe_e4_b1_224_eval"])
def test_step_equals_the_parent_path(tmp_path, name):
    """T + 3 steps of AgentStep against the parent path with the same seed, both modes: the control bit for bit, the frame ring
    equal; reset() starts an episode; a weight change is picked up on the next step without refresh()"""
    from pmoe_amd.infer import AgentStep
    model, meta, dev = _model(tmp_path, name)
    B, S = meta["batch"], meta["size"]
    sensor, crop = ((600, 800), (125, 90)) if S == 224 else ((100, 90), (5, 5))
    n_cmd = dev["command"].shape[1]
    options = [-1] + list(range(1, n_cmd + 1))                           # RoadOption values: VOID, then 1 .. n_commands
    rng = np.random.default_rng(7)
    for mode in ("eager", "plan"):
        agent = AgentStep(model, sensor=sensor, crop=crop, size=(S, S), batch=B, mode=mode, seed=5)
        parent = _ParentPath(model, B, crop, (S, S), mode, 5, n_cmd)
        assert agent.tick.T == parent.tick.T and agent.n_commands == n_cmd
        frames = _frames(B, sensor[0], sensor[1], 70)

        def both(i):
            bgra = next(frames)
            spds = rng.uniform(0.0, 9.0, B).tolist()
            cmds = [options[(i + b) % len(options)] for b in range(B)]
            sent = bgra if B > 1 or i % 2 else bgra[0]                  # [H0,W0,4] too where B = 1; numpy or CPU tensor
            got = agent.step(torch.from_numpy(sent.copy()) if i % 3 == 2 else sent, spds[0] if B == 1 else spds,
                             cmds[0] if B == 1 else cmds)
            want = parent.step(bgra, spds, cmds)
            assert got.dtype == np.float64 and got.shape == (B, 3)
            assert agent_ref.same_bits(got, want), (mode, i, got, want)
            assert torch.equal(agent.tick.frames, parent.tick.frames), (mode, i)
            for k in ("probs", "punet_actions", "raw"):
                a, b = getattr(agent.last, k), getattr(parent.tick.last, k)
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (mode, i, k)
        for i in range(agent.tick.T + 3):
            both(i)
        if parent.tick.moe is not None:
            assert agent.draws_done == parent.tick.draws_done == agent.tick.T + 3
        agent.reset()
        parent.tick.reset()
        assert not agent.tick.frames.any()
        both(100)
        assert not agent.tick.frames[:, :-1].any() or agent.tick.T == 1
        plan = agent.tick.plan
        with torch.no_grad():
            for p_ in model.parameters():
                p_.mul_(1.01)
        both(101)                                                        # no explicit refresh()
        both(102)
        if mode == "plan":
            assert plan is not None and agent.tick.plan is not plan
            assert agent.tick.plan.calls[0][0].__name__ == "pmoe_sensor_push"
            assert agent.tick.plan.calls[-1][0].__name__ == "pmoe_control_postprocess"
            assert len(agent.tick.plan.calls) == len(parent.tick.plan.calls) + 1
        else:
            assert plan is None
    with pytest.raises(ValueError, match="frame"):
        agent.step(np.zeros((B, sensor[0], sensor[1] // 2, 4), dtype=np.uint8), [1.0] * B, [1] * B)
    with pytest.raises(TypeError, match="uint8"):
        agent.step(np.zeros((B, sensor[0], sensor[1], 4), dtype=np.float32), [1.0] * B, [1] * B)
    with pytest.raises(ValueError, match="command"):
        agent.step(np.zeros((B, sensor[0], sensor[1], 4), dtype=np.uint8), [1.0] * B, [n_cmd + 1] * B)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        agent.step(np.zeros((B, sensor[0], sensor[1], 4), dtype=np.uint8), [1.0] * B, [1] * B)
