"""Host-side checks of the agent's step (pmoe_amd.infer.AgentStep): the control rule's numpy statement against its table, the
argument checks of the two entry points, the tile the wrapper picks, the errors raised before any device is touched and the
measurement arithmetic."""
import numpy as np
import pytest
import torch

from pmoe_amd import hip
from tests import agent_ref
from tests.test_abi import _declared

p1, p2, p3, p4, p5, p6, p7 = (0x1000 * k for k in range(1, 8))        # 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def test_control_ref_gives_the_table():
    for actions, want in agent_ref.CONTROL_TABLE:
        got = agent_ref.control_ref(np.array([actions], dtype=np.float32))
        assert got.dtype == np.float64 and got.shape == (1, 3)
        assert agent_ref.same_bits(got, np.array([want], dtype=np.float64)), (actions, got, want)
    # the floor is the double 0.4, not the f32 nearest to it; the f32 values are widened, not re-rounded
    assert agent_ref.control_ref(np.array([[0.0, 0.0]], dtype=np.float32))[0, 1] == 0.4 != float(np.float32(0.4))
    assert agent_ref.control_ref(np.array([[0.3, 0.5]], dtype=np.float32))[0, 0] == float(np.float32(0.3)) != 0.3
    whole = agent_ref.control_ref(np.array([a for a, _ in agent_ref.CONTROL_TABLE], dtype=np.float32))
    assert agent_ref.same_bits(whole, np.array([w for _, w in agent_ref.CONTROL_TABLE]))


def test_command_index_rule():
    assert [agent_ref.command_index(c) for c in (-1, 0, 1, 2, 3, 4, 5, 6)] == [3, 3, 0, 1, 2, 3, 4, 5]
    assert agent_ref.onehot_ref([-1, 2], 6).tolist() == [[0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 0]]


def test_library_exports_the_agent_kernels(lib):
    decl = _declared()
    for name, nargs in (("pmoe_sensor_push", 22), ("pmoe_control_postprocess", 4)):
        assert hasattr(lib, name), name
        assert decl[name] == nargs == len(hip.SIGNATURES[name])
        assert name not in hip._NOT_LAUNCHES
    assert lib.pmoe_version() == 401


# the agent's shape: 600 x 800 BGRA, crop (125, 90) -> 385 rows -> 224 x 224, tile of 8 output rows reading 16 source rows, bf16 NHWC
SENSOR_GOOD = [p1, p2, 1, 4, 600, 800, 125, 385, 224, 224, p3, p4, 9, p5, p6, 5, 8, 16, p7, 16, hip.DT_BF16, None]
SENSOR_REFUSED = ([{i: None} for i in (0, 1, 10, 11, 13, 14)] +                       # null pointers
                  [{0: p1 + 2}, {1: p2 + 2}] +                                         # pixels are dwords, the ring is f32
                  [{2: 0}, {2: 65536}, {3: 0}, {4: 0}, {5: 0}, {7: 0}, {8: 0}, {9: 0}, {12: 0}, {15: 0}, {17: 0}] +   # sizes
                  [{6: -1}, {6: 216}, {7: 476}, {6: 600}] +                           # the crop leaves the frame
                  [{16: 0}, {16: 3}, {16: 16}, {16: -8}] +                            # tile_rows outside {8, 4, 2, 1}
                  [{19: 2}, {19: 12}, {19: 0}, {18: p7 + 8}, {20: 7}, {20: hip.DT_F32, 19: 6}])   # Cp / dtype rules of pmoe_history_push


def _call(lib, name, good, change=None):
    args = list(good)
    for i, v in (change or {}).items():
        args[i] = v
    return getattr(lib, name)(*args)


# (with a GPU, a check that got lost would launch a kernel on the made-up pointers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="a lost check would launch on made-up device pointers")
def test_entry_points_refuse_what_the_host_can_check(lib):
    from pmoe_amd import ops
    from pmoe_amd.preprocess import _coeffs
    for change in SENSOR_REFUSED:
        assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, change) == hip.ERR_ARG, change
    # the accepted lists pass every check: without a GPU the launch behind them fails in the runtime with a HIP error > 0
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD) > 0
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {18: None, 19: 0, 20: 0}) > 0          # no NHWC copy: Cp / dtype unused
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {19: 4, 20: hip.DT_F32}) > 0
    for tile_rows in (4, 2, 1):
        assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {16: tile_rows}) > 0
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {17: 65536 // (224 * 3)}) > 0         # the last size that fits 64 KiB
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {17: 65536 // (224 * 3) + 1}) == hip.ERR_UNSUPPORTED
    # a 1200-row source -> 8 x 224: one output row reads 300 source rows, about 200 KB of resampled rows
    kv, bounds, _ = _coeffs(1200, 8)
    tile = ops.sensor_tile(bounds, 224)
    assert tile == (1, 300) and tile[1] * 224 * 3 > 3 * ops.SENSOR_LDS_BYTES
    tall = {4: 1200, 6: 0, 7: 1200, 8: 8, 15: kv, 16: tile[0], 17: tile[1]}
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, tall) == hip.ERR_UNSUPPORTED
    assert _call(lib, "pmoe_sensor_push", SENSOR_GOOD, {**tall, 0: None}) == hip.ERR_ARG    # (the argument checks come first)

    good = [p1, p2, 1, None]
    for change in ({0: None}, {1: None}, {2: 0}, {2: -3}):
        assert _call(lib, "pmoe_control_postprocess", good, change) == hip.ERR_ARG, change
    assert _call(lib, "pmoe_control_postprocess", good) > 0
    assert _call(lib, "pmoe_control_postprocess", good, {2: 1 << 20}) > 0


def test_tile_choice():
    from pmoe_amd import ops
    from pmoe_amd.preprocess import _coeffs

    def tile(rows, h, w):
        return ops.sensor_tile(_coeffs(rows, h)[1], w)
    # 400 x 48 -> 8 x 64: all eight rows read the whole source, 400 * 64 * 3 = 76 800 bytes > 64 KiB; four read 225 rows
    assert tile(400, 8, 64) == (4, 225)
    assert 400 * 64 * 3 > ops.SENSOR_LDS_BYTES >= 225 * 64 * 3
    # the agent: 600 x 800, crop (125, 90) -> 224 x 224
    assert tile(600 - 125 - 90, 224, 224) == (8, 16)
    # every choice covers its taps: from the first tap of a tile's first row to the last tap of any of its rows
    for rows, h, w in ((385, 224, 224), (291, 97, 65), (90, 224, 160), (140, 128, 128), (400, 8, 64), (1200, 8, 224), (7, 3, 5)):
        tr, tin = tile(rows, h, w)
        bounds = _coeffs(rows, h)[1]
        assert tr in (8, 4, 2, 1)
        for y0 in range(0, h, tr):
            first = bounds[y0][0]
            assert all(first <= lo and lo + n <= first + tin for lo, n in bounds[y0:y0 + tr])
        assert tin * w * 3 <= ops.SENSOR_LDS_BYTES or tr == 1
        for bigger in (t for t in (8, 4, 2) if t > tr):          # ... and it is the largest that fits
            need = max(max(lo + n for lo, n in bounds[y0:y0 + bigger]) - bounds[y0][0] for y0 in range(0, h, bigger))
            assert need * w * 3 > ops.SENSOR_LDS_BYTES


def _cpu_model():
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    return get_model(stage2_model_cfg("moe", 2, dropout=0.0))


def test_agent_step_refusals_before_any_device_call(monkeypatch):
    from pmoe_amd import infer

    def no_device(*a, **k):
        raise AssertionError("AgentStep touched the device layer before validating its arguments")
    monkeypatch.setattr(hip, "load", no_device)
    model = _cpu_model()
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        infer.AgentStep(model)
    model.eval()
    with pytest.raises(ValueError, match="mode"):
        infer.AgentStep(model, mode="graph")
    with pytest.raises(ValueError, match="no rows"):
        infer.AgentStep(model, sensor=(200, 800), crop=(125, 90))
    with pytest.raises(ValueError, match="no rows"):
        infer.AgentStep(model, sensor=(215, 800), crop=(125, 90))
    with pytest.raises(RuntimeError, match="no CPU path"):
        infer.AgentStep(model)
    with pytest.raises(TypeError):
        infer.AgentStep(torch.nn.Linear(2, 2).eval())


def test_measurements_follow_the_reference_arithmetic():
    from pmoe_amd.infer import AgentStep
    # a command out of range: where the reference's scatter_ fails
    for cmd, n in ((7, 6), (5, 4), (-1, 3), (0, 2)):
        with pytest.raises(ValueError, match="command"):
            AgentStep.measurements(1.0, cmd, 1, 10.0, n)
    with pytest.raises(ValueError):
        AgentStep.measurements([1.0, 2.0], 1, 2, 10.0, 6)              # B speeds need B commands
    with pytest.raises(TypeError):
        AgentStep.measurements(1.0, 2.0, 1, 10.0, 6)
    cmds = [-1, 0, 1, 2, 3, 4, 5, 6]
    speed, onehot = AgentStep.measurements(np.linspace(0.0, 9.0, len(cmds)), cmds, len(cmds), 10.0, 6)
    assert onehot.dtype == np.float32 and np.array_equal(onehot, agent_ref.onehot_ref(cmds, 6))
    assert speed.dtype == np.float32 and speed.shape == (len(cmds),)
    # the speed: divided in double, rounded to f32 once (torch.tensor([spd / 10.0], dtype=torch.float), image_agent.py:151-153).
    # A quotient of two f32 numbers rounds the same either way, so the difference is whether spd is rounded before the division.
    for spd in (0.039, 0.13, 7.3100000000000005):
        once = np.float32(spd / 10.0)
        got, _ = AgentStep.measurements(spd, 4, 1, 10.0, 6)
        assert got[0] == once == torch.tensor([spd / 10.0], dtype=torch.float)[0].item()
    differ = [spd for spd in (0.039, 0.13) if np.float32(np.float32(spd) / np.float32(10.0)) != np.float32(spd / 10.0)]
    assert differ == [0.039, 0.13]                                      # (the values above do tell the two apart)
    assert AgentStep.measurements(np.float32(3.3), 4, 1, 10.0, 6)[0][0] == np.float32(float(np.float32(3.3)) / 10.0)
