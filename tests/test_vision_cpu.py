"""Host-side checks of pmoe_amd.vision: the numpy restatement (tests/vision_ref.py) against the reference's recorded outputs
(tests/golden/vision.npz, tools/make_vision_golden.py), the integer "%.3f" against Python's, the font table, the argument checks
of the two entry points and the errors raised before any device is touched."""
from pathlib import Path

import numpy as np
import pytest
import torch

from pmoe_amd import hip, vision
from tests import vision_ref
from tests.test_abi import _declared

GOLDEN = Path(__file__).resolve().parent / "golden" / "vision.npz"
p1, p2, p3, p4, p5, p6, p7, p8 = (0x1000 * k for k in range(1, 9))     # 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip.load()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_vision_ref_equals_the_reference_outputs():
    fx = np.load(GOLDEN)
    assert fx["logits"].shape == (23, 12, 16) and fx["ids"].shape == (12, 16) and fx["frames"].shape == (2, 3, 20, 28)
    assert {22, 23, 255} <= set(fx["ids"].reshape(-1).tolist())
    assert same_bits(vision_ref.decode_mask_ref(fx["logits"]), fx["logits_rgb"])
    assert same_bits(vision_ref.decode_mask_ref(fx["ids"]), fx["ids_rgb"])
    assert same_bits(vision_ref.decode_mask_ref(fx["ids"], nc=5), fx["ids_rgb_nc5"])
    assert same_bits(vision_ref.decode_mask_ref(fx["ids"].astype(np.uint8)), fx["ids_rgb"])
    assert fx["logits_rgb"].dtype == np.float64 and fx["ids_rgb_nc5"].any() and not fx["ids_rgb"][:, 0, 1:3].any()
    # the planted ties took the lower index
    ids = np.argmax(fx["logits"], axis=0)
    assert (ids[0, 0], ids[0, 1], ids[5, 7], ids[11, 15]) == (3, 0, 21, 0)
    for frame, want in zip(fx["frames"], fx["frames_u8"]):
        assert same_bits(vision_ref.normalise_ref(frame), want)
    # the palette is the documented one: 23 classes, and the f32 / uint8 forms follow from it
    assert tuple(vision.CARLA_PALETTE.shape) == (23, 3) and vision.CARLA_PALETTE.dtype == torch.uint8
    u8 = vision_ref.decode_mask_ref(fx["ids"], dtype=np.uint8)
    assert u8.shape == (12, 16, 3) and np.array_equal(u8.transpose(2, 0, 1) / 255.0, fx["ids_rgb"])
    f32 = vision_ref.decode_mask_ref(fx["ids"], dtype=np.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255))


def test_normalise_ref_edge_cases():
    const = np.full((3, 4, 5), 2.5, dtype=np.float32)
    assert not vision_ref.normalise_ref(const).any()
    img = np.arange(60, dtype=np.float32).reshape(3, 4, 5)
    img[1, 2, 3] = np.nan
    out = vision_ref.normalise_ref(img)
    assert out[2, 3, 1] == 0 and out[0, 0, 0] == 0 and out[3, 4, 2] == 255          # the NaN is no extremum
    assert not vision_ref.normalise_ref(np.full((3, 2, 2), np.nan, dtype=np.float32)).any()


def fmt3_values():
    """the f32 values whose "%.3f" both suites check"""
    vals = [np.float32(k / 16) for k in range(-64, 65)] + [np.float32(0.0), np.float32(-0.0)]
    for k in range(-4000, 4001):                                  # the rounding boundaries k / 2000 and their f32 neighbours
        x = np.float32(k / 2000)
        vals += [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000, 0x80000001, 0x807FFFFF], dtype=np.uint32).view(np.float32)     # denormals, the first normal
    vals += list(tiny) + [np.float32(1048575.9375), np.float32(-1048575.9375), np.float32(np.nan), np.float32(np.inf),
                          np.float32(-np.inf)]
    return np.array(vals, dtype=np.float32)


def test_fmt3_is_pythons():
    vals = fmt3_values()
    assert len(vals) > 24000
    for x in vals:
        assert vision_ref.fmt3(x) == "%.3f" % float(x), (x, vision_ref.fmt3(x))
    assert vision_ref.fmt3(np.float32(-0.0)) == "-0.000" and vision_ref.fmt3(np.float32(-0.0004)) == "-0.000"
    assert vision_ref.fmt3(np.float32(0.0625)) == "0.062" and vision_ref.fmt3(np.float32(0.1875)) == "0.188"   # ties to even
    assert vision_ref.fmt3(np.float32(2.0 ** 20)) == "big" and vision_ref.fmt3(np.float32(-3e9)) == "-big"
    assert max(len(s) for s in vision_ref.strings_ref((-1048575.9375, -1048575.9375), [1.0])) <= vision.TEXT_COLS


def test_strings_follow_the_reference_rules():
    rows = vision_ref.strings_ref((0.5, 0.25), [0, 0, 1, 0], 0.5, (-0.125, -0.75), gt=True)
    assert rows == ["Steer: 0.500", "Throttle: 0.250", "Brake: 0.000", "Command: 2", "Speed: 0.500", "Steer: -0.125",
                    "Throttle: 0.000", "Brake: 0.750"]
    assert vision_ref.strings_ref((0.0, 0.0), [1, 1])[1:4] == ["Throttle: 0.000", "Brake: -0.000", "Command: 0"]
    assert vision_ref.strings_ref((0.0, -0.0), [0, 1])[1:3] == ["Throttle: 0.000", "Brake: 0.000"]
    assert vision_ref.strings_ref((0.0, np.nan), [0, 1])[1:3] == ["Throttle: 0.000", "Brake: nan"]
    assert vision_ref.strings_ref((0.0, 0.0), [0, 1])[4:] == [""] * 4
    assert vision_ref.text_codes(rows).shape == (vision.TEXT_ROWS, vision.TEXT_COLS) == (8, 24)


def test_font_covers_the_strings():
    for ch, masks in vision.FONT.items():
        assert len(ch) == 1 and ord(ch) < 128 and len(masks) == 7 and all(0 <= m < 32 for m in masks), ch
    needed = set("Steer: Throttle: Brake: Command: Speed: 0123456789.-naninfbig")
    assert needed <= set(vision.FONT), needed - set(vision.FONT)
    assert not any(vision.FONT[" "]) and all(any(m) for ch, m in vision.FONT.items() if ch != " ")
    assert len({m for m in vision.FONT.values()}) == len(vision.FONT)               # no two glyphs alike


def test_library_exports_the_vision_kernels(lib):
    decl = _declared()
    for name, nargs in (("pmoe_decode_mask", 11), ("pmoe_frame_annotate", 17)):
        assert hasattr(lib, name), name
        assert decl[name] == nargs == len(hip.SIGNATURES[name])
        assert name not in hip._NOT_LAUNCHES
    assert lib.pmoe_version() == 401


# mask, kind, out, out_dtype, palette, nc, B, C, H, W, stream
DECODE_GOOD = [p1, 0, p2, 2, p3, 23, 4, 23, 12, 16, None]
DECODE_REFUSED = ([{0: None}, {2: None}, {4: None}] +                                       # null pointers
                  [{0: p1 + 2}, {1: 1, 0: p1 + 4}, {2: p2 + 4}, {3: 1, 2: p2 + 2}] +        # f32 / int64 / f64 / f32 alignment
                  [{5: 0}, {5: -1}, {6: 0}, {6: 65536}, {7: 0}, {8: 0}, {9: 0}, {9: -4}] +  # nc, B, C, H, W
                  [{1: 3}, {1: -1}, {3: 3}, {3: -1}] +                                      # unknown kind / dtype code
                  [{8: 1 << 15, 9: 1 << 14}])                                               # H W > 2^28
# frames, stride, out, B, H, W, slot0, capacity, action, speed, command, n_cmd, control_gt, gt, font, text_out, stream
ANNOT_GOOD = [p1, 4 * 3 * 224 * 224, p2, 3, 224, 224, 998, 1000, p3, p4, p5, 6, p6, 1, p7, p8, None]
ANNOT_REFUSED = ([{i: None} for i in (0, 2, 8, 9, 10, 12, 14)] +                            # null pointers (gt reads all)
                 [{0: p1 + 2}, {8: p3 + 1}, {9: p4 + 2}, {10: p5 + 3}, {12: p6 + 2}] +      # f32 alignment
                 [{3: 0}, {3: 65536, 7: 70000}, {4: 0}, {5: 0}, {5: -224}, {11: 0}, {7: 0}] +   # sizes, B > 65535
                 [{3: 5, 7: 4, 6: 0}, {6: -1}, {6: 1000}, {1: 3 * 224 * 224 - 1}, {4: 1 << 15, 5: 1 << 14, 1: 1 << 62}])


def _call(lib, name, good, change=None):
    args = list(good)
    for i, v in (change or {}).items():
        args[i] = v
    return getattr(lib, name)(*args)


# (with a GPU, a check that got lost would launch a kernel on the made-up pointers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="a lost check would launch on made-up device pointers")
def test_entry_points_refuse_what_the_host_can_check(lib):
    for change in DECODE_REFUSED:
        assert _call(lib, "pmoe_decode_mask", DECODE_GOOD, change) == hip.ERR_ARG, change
    for change in ANNOT_REFUSED:
        assert _call(lib, "pmoe_frame_annotate", ANNOT_GOOD, change) == hip.ERR_ARG, change
    # the accepted lists pass every check: without a GPU the launch behind them fails in the runtime with a HIP error > 0
    assert _call(lib, "pmoe_decode_mask", DECODE_GOOD) > 0
    for change in ({1: 1, 7: 0}, {1: 2, 0: p1 + 1, 7: 0}, {3: 0, 2: p2 + 1}, {3: 1, 2: p2 + 4}, {6: 65535}, {5: 1}):
        assert _call(lib, "pmoe_decode_mask", DECODE_GOOD, change) > 0, change
    assert _call(lib, "pmoe_frame_annotate", ANNOT_GOOD) > 0
    # gt = 0 reads neither the speed nor the ground truth; text_out is optional; odd frames and bases take the scalar path
    for change in ({13: 0, 9: None, 12: None}, {15: None}, {4: 33, 5: 47, 1: 3 * 33 * 47}, {0: p1 + 4, 2: p2 + 1}, {3: 1000, 6: 0},
                   {3: 65535, 7: 65535, 6: 0}):
        assert _call(lib, "pmoe_frame_annotate", ANNOT_GOOD, change) > 0, change


def test_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        vision.decode_mask(torch.zeros(23, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        vision.decode_mask(torch.zeros(4, 4, dtype=torch.int64), nc=5, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vision.draw_on_image(torch.zeros(3, 8, 8), {"command": torch.zeros(6)}, torch.zeros(2), gt=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vision.FrameLog(capacity=4, size=(8, 8), device="cpu")
    with pytest.raises(ValueError, match="positive"):
        vision.FrameLog(capacity=0, size=(8, 8))


def test_agent_step_checks_its_log_before_any_device_call(monkeypatch):
    """a log of another size is refused on the host; without a log the construction is what it was"""
    from pmoe_amd import infer
    from tests.test_agent_step_cpu import _cpu_model

    def no_device(*a, **k):
        raise AssertionError("AgentStep touched the device layer before validating its arguments")
    monkeypatch.setattr(hip, "load", no_device)
    model = _cpu_model().eval()
    log = vision.FrameLog.__new__(vision.FrameLog)
    log.capacity, log.size = 4, (32, 32)
    with pytest.raises(ValueError, match="FrameLog"):
        infer.AgentStep(model, size=(64, 64), log=log)
    with pytest.raises(TypeError, match="FrameLog"):
        infer.AgentStep(model, size=(64, 64), log=[])
    log.size, log.capacity = (64, 64), 1
    with pytest.raises(ValueError, match="capacity"):
        infer.AgentStep(model, size=(64, 64), batch=2, log=log)
