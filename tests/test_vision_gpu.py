"""pmoe_amd.vision on the device against its numpy restatement (tests/vision_ref.py) and the reference's recorded outputs
(tests/golden/vision.npz), bit for bit: decode_mask, draw_on_image, the formatted strings, FrameLog and AgentStep(log=...)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import vision_ref
from tests.test_vision_cpu import fmt3_values

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "vision.npz"
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- decode_mask
def test_decode_mask_equals_the_reference_arrays():
    from pmoe_amd import vision
    fx = np.load(GOLDEN)
    assert torch.equal(vision.decode_mask(_dev(fx["logits"])).cpu(), torch.from_numpy(fx["logits_rgb"]))
    assert torch.equal(vision.decode_mask(_dev(fx["ids"])).cpu(), torch.from_numpy(fx["ids_rgb"]))
    assert torch.equal(vision.decode_mask(_dev(fx["ids"]), nc=5).cpu(), torch.from_numpy(fx["ids_rgb_nc5"]))
    assert torch.equal(vision.decode_mask(_dev(fx["ids"].astype(np.uint8))).cpu(), torch.from_numpy(fx["ids_rgb"]))
    assert vision.decode_mask(_dev(fx["logits"])).dtype == torch.float64


def test_decode_mask_batched_ties_and_nan():
    from pmoe_amd import vision
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((2, 23, 33, 47)).astype(np.float32)
    logits[0, [4, 19], 5, 6] = 11.0                               # a tie of two maxima
    logits[1, :, 32, 46] = -1.5                                   # all equal, at the last pixel
    logits[0, [20, 22], 0, 0] = 12.0
    logits[1, [7, 15], 10, 20] = np.nan                           # the first NaN wins, also over a larger value
    logits[1, 3, 10, 20] = 50.0
    ids = np.argmax(logits, axis=1)
    assert (ids[0, 5, 6], ids[1, 32, 46], ids[0, 0, 0], ids[1, 10, 20]) == (4, 0, 20, 7)
    for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32), (torch.uint8, np.uint8)):
        for nc in (23, 9):
            got = vision.decode_mask(_dev(logits), nc=nc, dtype=tdt)
            want = vision_ref.decode_mask_ref(logits, nc=nc, dtype=ndt)
            assert got.dtype == tdt and tuple(got.shape) == want.shape == ((2, 33, 47, 3) if ndt == np.uint8 else (2, 3, 33, 47))
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (tdt, nc)
    # ids as int64 and as uint8; out-of-range ones are black; leading dimensions are kept
    raw = rng.integers(0, 30, (2, 2, 33, 47)).astype(np.int64)
    raw[0, 0, 0, :3] = (-1, 255, 22)
    a = vision.decode_mask(_dev(raw))
    b = vision.decode_mask(_dev((raw & 0xFF).astype(np.uint8)))
    want = vision_ref.decode_mask_ref(raw)
    assert tuple(a.shape) == (2, 2, 3, 33, 47) and torch.equal(a.cpu(), torch.from_numpy(want))
    raw[0, 0, 0, 0] = 255                                         # (what -1 becomes as a byte: black either way)
    assert torch.equal(b.cpu(), torch.from_numpy(vision_ref.decode_mask_ref(raw)))
    # a palette of the caller's
    pal = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    got = vision.decode_mask(_dev(raw), nc=7, palette=_dev(pal), dtype=torch.uint8)
    assert torch.equal(got.cpu(), torch.from_numpy(vision_ref.decode_mask_ref(raw, nc=7, palette=pal, dtype=np.uint8)))
    with pytest.raises(ValueError, match="palette"):
        vision.decode_mask(_dev(raw), nc=8, palette=_dev(pal))


# ---- draw_on_image
ACTIONS = np.array([[0.5, 0.0], [-0.25, -0.0], [0.001, np.nan], [-1.0, -0.7], [0.3333, 0.6]], dtype=np.float32)


def _measurements(rng, b, n_cmd=6):
    command = np.zeros((b, n_cmd), dtype=np.float32)
    command[np.arange(b), rng.integers(0, n_cmd, b)] = 1.0
    control = rng.uniform(-1, 1, (b, 2)).astype(np.float32)
    speed = rng.uniform(0, 9, (b, 1)).astype(np.float32)
    return dict(control=control, speed=speed, command=command)


def _draw_both(frames, meas, action, gt):
    from pmoe_amd import vision
    dmeas = {k: _dev(v) for k, v in meas.items()} if gt else {"command": _dev(meas["command"])}
    got = vision.draw_on_image(_dev(frames), dmeas, _dev(action), gt=gt)
    want = np.stack([vision_ref.draw_ref(f, a, c, s, g, gt)
                     for f, a, c, s, g in zip(frames, action, meas["command"], meas["speed"], meas["control"])])
    return got, want


@pytest.mark.parametrize("hw", [(80, 100), (33, 47), (224, 224)])
def test_draw_on_image_equals_its_statement(hw):
    rng = np.random.default_rng(hw[0])
    h, w = hw
    frames = (rng.standard_normal((3, 3, h, w)) * 0.3 + 0.4).astype(np.float32)
    meas = _measurements(rng, 3)
    for gt in (True, False):
        for action in (ACTIONS[:3], ACTIONS[2:5]):
            got, want = _draw_both(frames, meas, action, gt)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w, 3)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (hw, gt)
    # the text is there and clipped: ink in the first string's box where the frame has it
    box = want[0][30:37, 5:5 + 6 * 12]
    assert ((box == vision_ref.RED).all(-1)).any() == (h > 30)


def test_draw_on_image_edge_frames_and_single_frame():
    from pmoe_amd import vision
    rng = np.random.default_rng(5)
    frames = rng.standard_normal((3, 3, 33, 47)).astype(np.float32)
    frames[0] = 1.25                                              # a constant frame: 0 everywhere under the text
    frames[1, 2, 20, 11] = np.nan                                 # a NaN pixel: 0, and no extremum
    frames[2, :, :, 0] = 3.0e38
    meas = _measurements(rng, 3)
    got, want = _draw_both(frames, meas, ACTIONS[:3], True)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    plain = vision_ref.normalise_ref(frames[0])
    assert not plain.any() and want[1, 20, 11, 2] == 0 and want[1].max() == 255
    # [3,H,W] in, [H,W,3] out, unbatched measurements, speed without a dimension
    one = vision.draw_on_image(_dev(frames[1]), dict(control=_dev(meas["control"][1]), speed=_dev(meas["speed"][1, 0]),
                                                     command=_dev(meas["command"][1])), _dev(ACTIONS[1]), gt=True)
    assert tuple(one.shape) == (33, 47, 3) and torch.equal(one.cpu(), torch.from_numpy(want[1]))
    with pytest.raises(KeyError):
        vision.draw_on_image(_dev(frames[1]), {"command": _dev(meas["command"][1])}, _dev(ACTIONS[1]), gt=True)


def test_fixture_frames_equal_the_reference_outside_the_text():
    from pmoe_amd import vision
    fx = np.load(GOLDEN)
    frames = fx["frames"]
    rng = np.random.default_rng(1)
    meas = _measurements(rng, 2)
    region = vision_ref.text_region(20, 28)
    assert region.any() and not region.all()
    for gt in (True, False):
        got, _ = _draw_both(frames, meas, ACTIONS[:2], gt)
        got = got.cpu().numpy()
        for g, want in zip(got, fx["frames_u8"]):
            assert np.array_equal(g[~region], want[~region])


# ---- the formatted strings
def test_formatted_numbers_are_pythons():
    from pmoe_amd import vision
    listed = fmt3_values()
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 1 << 32, 1 << 17, dtype=np.uint64).astype(np.uint32)
    bits = bits[((bits >> 23) & 0xFF) < 127 + 20][:65536 - len(listed)]          # |x| < 2^20
    values = np.concatenate([listed, bits.view(np.float32)])
    assert values.shape == (65536,)
    b = 4096
    frames = torch.zeros(b, 3, 8, 8, device=DEV)
    out = torch.empty(b, 8, 8, 3, dtype=torch.uint8, device=DEV)
    command = torch.zeros(b, 1, device=DEV)
    text = torch.zeros(16, b, vision.TEXT_ROWS, vision.TEXT_COLS, dtype=torch.uint8, device=DEV)
    for i in range(16):
        action = np.stack([values[i * b:(i + 1) * b], np.ones(b, dtype=np.float32)], axis=1)
        vision.annotate(frames, out, _dev(action), command, text_out=text[i])
    text = text.cpu().numpy().reshape(65536, vision.TEXT_ROWS, vision.TEXT_COLS)
    for x, rows in zip(values, text):
        got = bytes(rows[0]).decode()
        assert got == ("Steer: %.3f" % float(x)).ljust(vision.TEXT_COLS), (x, got)
    assert bytes(text[0, 1]).decode().rstrip() == "Throttle: 1.000" and bytes(text[0, 3]).decode().rstrip() == "Command: 0"
    assert not (text[:, 4:] != ord(" ")).any()
    # beyond the range: "big" / "-big", and the infinities
    action = _dev(np.array([[2.0 ** 20, 1], [-3.0e9, 1], [np.inf, 1], [-np.inf, 1]], dtype=np.float32))
    t4 = torch.zeros(4, vision.TEXT_ROWS, vision.TEXT_COLS, dtype=torch.uint8, device=DEV)
    vision.annotate(frames[:4], out, action, command[:4], text_out=t4)
    assert [bytes(r[0]).decode().rstrip() for r in t4.cpu().numpy()] == ["Steer: big", "Steer: -big", "Steer: inf", "Steer: -inf"]


# ---- FrameLog
def test_frame_log_ring():
    from pmoe_amd import vision
    rng = np.random.default_rng(9)
    frames = rng.standard_normal((12, 3, 16, 20)).astype(np.float32)
    meas = _measurements(rng, 12)
    action = rng.uniform(-1, 1, (12, 2)).astype(np.float32)
    want_gt = np.stack([vision_ref.draw_ref(frames[i], action[i], meas["command"][i], meas["speed"][i], meas["control"][i], True)
                        for i in range(12)])
    want = np.stack([vision_ref.draw_ref(frames[i], action[i], meas["command"][i]) for i in range(12)])
    d = {k: _dev(v) for k, v in meas.items()}
    dframes, daction = _dev(frames), _dev(action)

    log = vision.FrameLog(capacity=5, size=(16, 20), device=DEV)
    assert len(log) == 0 and log.dropped == 0 and log.frames().shape == (0, 16, 20, 3)
    for i in range(7):
        log.push(dframes[i:i + 1], daction[i:i + 1], d["speed"][i:i + 1], d["command"][i:i + 1])
        assert len(log) == min(i + 1, 5)
    got = log.frames()
    assert got.dtype == np.uint8 and np.array_equal(got, want[2:7]) and log.dropped == 2
    log.clear()
    assert len(log) == 0 and log.dropped == 0 and log.frames().shape == (0, 16, 20, 3)
    log.push(dframes[:2], daction[:2], d["speed"][:2], d["command"][:2], control_gt=d["control"][:2])
    assert np.array_equal(log.frames(), want_gt[:2])

    log = vision.FrameLog(capacity=6, size=(16, 20), device=DEV)
    for i in range(0, 12, 4):                                     # the second push wraps inside its launch
        log.push(dframes[i:i + 4], daction[i:i + 4], d["speed"][i:i + 4], d["command"][i:i + 4], control_gt=d["control"][i:i + 4])
        assert np.array_equal(log.frames(), want_gt[max(0, i + 4 - 6):i + 4])
    assert len(log) == 6 and log.dropped == 6
    with pytest.raises(ValueError):
        log.push(dframes[:7], daction[:7], d["speed"][:7], d["command"][:7])
    with pytest.raises(ValueError):
        log.push(_dev(frames[:1, :, :8]), daction[:1], d["speed"][:1], d["command"][:1])


# ---- AgentStep(log=...)
def test_agent_step_logs_what_draw_on_image_draws():
    from pmoe_amd import vision
    from pmoe_amd.infer import AgentStep
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    torch.manual_seed(0)
    model = get_model(stage2_model_cfg("moe", 2, dropout=0.0)).to(DEV).eval()
    sensor, crop, size, b = (120, 160), (25, 18), (64, 64), 2
    rng = np.random.default_rng(4)
    steps = [(rng.integers(0, 256, (b,) + sensor + (4,), dtype=np.uint8), rng.uniform(0, 9, b).tolist(), [1 + (i + k) % 4 for k in range(b)])
             for i in range(3)]
    with pytest.raises(ValueError, match="FrameLog"):
        AgentStep(model, sensor=sensor, crop=crop, size=size, batch=b, log=vision.FrameLog(4, (32, 32), DEV))
    for mode in ("plan", "eager"):
        plain = AgentStep(model, sensor=sensor, crop=crop, size=size, batch=b, mode=mode, seed=3)
        log = vision.FrameLog(capacity=8, size=size, device=DEV)
        agent = AgentStep(model, sensor=sensor, crop=crop, size=size, batch=b, mode=mode, seed=3, log=log)
        assert plain.log is None
        if mode == "plan":
            assert len(agent.tick.plan.calls) == len(plain.tick.plan.calls)
            assert [c[0].__name__ for c in agent.tick.plan.calls] == [c[0].__name__ for c in plain.tick.plan.calls]
        want = []
        for bgra, spd, cmd in steps:
            got = agent.step(bgra, spd, cmd)
            assert np.array_equal(got, plain.step(bgra, spd, cmd))
            tick = agent.tick
            actions = tick.out if tick.pun is not None and tick.moe is not None else tick.raw
            want.append(vision.draw_on_image(tick.frames[:, -1], {"command": tick.static_in[2]}, actions, gt=False).cpu().numpy())
        assert len(log) == 6 and log.dropped == 0
        assert np.array_equal(log.frames(), np.concatenate(want))
        assert (np.concatenate(want) == vision_ref.GREEN).all(-1).any()          # the command row is drawn with gt=False
