"""Train-time augmenter on the GPU (pmoe_amd/augment.py, csrc/augment.hip) against its numpy restatement (tests/augment_ref.py)
with hand-built plans: bit exact for every operator but the Gaussian noise, which is checked by its moments."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.make_prep_golden import CASES, frame  # noqa: E402
from pmoe_amd import augment, hip  # noqa: E402
from pmoe_amd.augment import AugmentPlan, get_augmenter  # noqa: E402
from pmoe_amd.preprocess import FramePreprocessor  # noqa: E402
from tests import augment_ref as ref  # noqa: E402

AUG = get_augmenter()            # __call__ with plan= never looks at the schedule


def _frames(n, h, w, seed=0):
    """random frames, then the clamp / tie cases written over the first rows: all 0, all 255 and a 0..255 ramp"""
    x = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    flat = x.reshape(n, -1)
    flat[0, :] = (np.arange(flat.shape[1]) * 7 // 3) % 256                 # every value 0..255, in all three channels
    if n > 1:
        flat[1, : flat.shape[1] // 3] = 0
        flat[1, flat.shape[1] // 3: 2 * flat.shape[1] // 3] = 255
    return x


def _edge_batches(n, h, w):
    """whole frames of all 0, all 255 and a 0..255 ramp (clamp and tie cases), in batches of n"""
    ramp = (np.arange(h * w * 3) % 256).astype(np.uint8).reshape(h, w, 3)
    kinds = [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), ramp]
    for k in range(0, 3, n):
        yield np.stack([kinds[(k + i) % 3] for i in range(n)])


SHAPES = {"3x19x37": (3, 19, 37), "2x16x16": (2, 16, 16)}


def _run(x, plan):
    got = AUG(torch.from_numpy(x).cuda(), plan=plan)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    return got.cpu().numpy()


def _check(x, slots_per_frame):
    n, h, w, _ = x.shape
    plan = AugmentPlan.from_slots(slots_per_frame, h, w)
    want = ref.apply_plan(x, plan)
    got = _run(x, plan)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return want


POINT_CASES = [
    ("add+255", {"op": "add", "p": 255}), ("add-255", {"op": "add", "p": -255}), ("add0", {"op": "add", "p": 0}),
    ("add_pc", {"op": "add", "p": (40, -17, 3)}),
    ("mul0", {"op": "multiply", "p": 0.0}), ("mul1", {"op": "multiply", "p": 1.0}), ("mul1.5", {"op": "multiply", "p": 1.5}),
    ("mul2.5", {"op": "multiply", "p": 2.5}), ("mul_pc", {"op": "multiply", "p": (0.5, 1.5, 1.2999999523162842)}),
    ("con0", {"op": "contrast", "p": 0.0}), ("con0.5", {"op": "contrast", "p": 0.5}), ("con1.5", {"op": "contrast", "p": 1.5}),
    ("con_pc", {"op": "contrast", "p": (0.5, 1.5, 0.7300000190734863)}),
    ("gray0", {"op": "grayscale", "p": 0.0}), ("gray0.5", {"op": "grayscale", "p": 0.5}), ("gray1", {"op": "grayscale", "p": 1.0}),
    ("drop0", {"op": "dropout", "p": 0.0, "seed": 11}), ("drop1", {"op": "dropout", "p": 1.0, "seed": 11}),
    ("drop0.3", {"op": "dropout", "p": 0.3, "seed": 2 ** 62 + 12345}),
    ("drop0.3_pc", {"op": "dropout", "p": 0.3, "per_channel": 1, "seed": 2 ** 62 + 12345}),
    ("drop1_pc", {"op": "dropout", "p": 1.0, "per_channel": 1, "seed": 3}),
    ("coarse3x3", {"op": "coarse_dropout", "p": 0.4, "hl": 3, "wl": 3, "seed": 99}),
    ("coarse3x3_pc", {"op": "coarse_dropout", "p": 0.4, "hl": 3, "wl": 3, "per_channel": 1, "seed": 99}),
    ("coarse_full", {"op": "coarse_dropout", "p": 0.4, "hl": None, "wl": None, "seed": 5}),
    ("coarse_full_pc", {"op": "coarse_dropout", "p": 0.4, "hl": None, "wl": None, "per_channel": 1, "seed": 5}),
    ("blur5", {"op": "blur", "sigma": 1.0}), ("blur7", {"op": "blur", "sigma": 2.2}), ("blur9", {"op": "blur", "sigma": 2.8}),
]


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
@pytest.mark.parametrize("case", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_each_operator_alone_is_bit_exact(shape, case):
    n, h, w = SHAPES[shape]
    slot = dict(case[1])
    if slot["op"] == "coarse_dropout" and slot["hl"] is None:
        slot["hl"], slot["wl"] = h, w                                        # hl x wl = h x w: the cell is the pixel
    x = _frames(n, h, w, seed=1)
    want = _check(x, [[slot]] * n)
    for e in _edge_batches(n, h, w):
        _check(e, [[slot]] * n)
    if slot["op"] == "blur":
        assert len(augment.blur_taps(slot["sigma"])) == int(case[0][4:])
    if case[0] in ("add0", "mul1", "gray0", "drop0"):
        assert np.array_equal(want, x)
    if case[0] in ("mul0", "drop1", "drop1_pc"):
        assert not want.any()
    if case[0] == "coarse_full":                                             # = DROPOUT with the same seed: one rule
        plain = AugmentPlan.from_slots([[{"op": "dropout", "p": 0.4, "seed": 5}]] * n, h, w)
        assert np.array_equal(want, ref.apply_plan(x, plain))
    if case[0] in ("drop0.3", "coarse3x3"):                                  # shared mask: a pixel is dropped as a whole
        dropped = (want == 0) & (x != 0)
        assert dropped.any() and (dropped | (x == 0)).all(-1)[dropped.any(-1)].all()


def test_blur_reflects_at_both_borders_of_one_row():
    """5 x 6 with K = 9: the halo of 4 reflects at the left AND the right border of every row, and at top and bottom"""
    x = _frames(2, 5, 6, seed=3)
    assert len(augment.blur_taps(2.8, 5, 6)) == 9
    _check(x, [[{"op": "blur", "sigma": 2.8}]] * 2)


def test_blur_across_tile_borders():
    """wider and taller than one block's tile of either pass (128 columns x 4 rows, 64 columns x 32 rows), odd sizes, K = 33"""
    x = _frames(2, 45, 150, seed=4)
    _check(x, [[{"op": "blur", "sigma": 13.0}], [{"op": "blur", "sigma": 1.0}]])


def test_order_matters():
    x = _frames(1, 19, 37, seed=2)
    a = _check(x, [[{"op": "add", "p": 40}, {"op": "multiply", "p": 2.5}]])
    b = _check(x, [[{"op": "multiply", "p": 2.5}, {"op": "add", "p": 40}]])
    assert not np.array_equal(a, b)


MIXED = [
    [{"op": "blur", "sigma": 1.0}, {"op": "add", "p": (30, -30, 5)}, {"op": "dropout", "p": 0.2, "per_channel": 1, "seed": 7}],
    [{"op": "multiply", "p": 1.5}, {"op": "coarse_dropout", "p": 0.3, "hl": 4, "wl": 5, "seed": 8}, {"op": "blur", "sigma": 2.2},
     {"op": "contrast", "p": (0.5, 1.5, 1.0)}, {"op": "grayscale", "p": 0.5}],
    [{"op": "grayscale", "p": 1.0}, {"op": "add", "p": -20}, {"op": "blur", "sigma": 2.8}],
    [{"op": "contrast", "p": 1.5}, {"op": "dropout", "p": 0.1, "seed": 9}, {"op": "add", "p": 12}, {"op": "multiply", "p": 0.75},
     {"op": "grayscale", "p": 0.25}, {"op": "coarse_dropout", "p": 0.2, "hl": 3, "wl": 3, "per_channel": 1, "seed": 10},
     {"op": "contrast", "p": 0.5}, {"op": "add", "p": 1}],
]


def test_phase_split_around_the_blur():
    """one batch: blur in slot 0, blur in the middle, blur last, no blur (with all 8 slots in use)"""
    x = _frames(4, 19, 37, seed=5)
    _check(x, MIXED)
    with hip.LaunchRecorder() as rec:
        _run(x, AugmentPlan.from_slots(MIXED, 19, 37))
    assert [fn.__name__ for fn, _ in rec.calls] == ["pmoe_augment_point_to_u8", "pmoe_augment_blur_h", "pmoe_augment_blur_v",
                                                    "pmoe_augment_point_to_u8"]


def test_no_blur_in_the_batch_means_no_blur_launches():
    x = _frames(2, 16, 16, seed=6)
    plan = AugmentPlan.from_slots([MIXED[3], [{"op": "add", "p": 3}]], 16, 16)
    with hip.LaunchRecorder() as rec:
        got = _run(x, plan)
    assert [fn.__name__ for fn, _ in rec.calls] == ["pmoe_augment_point_to_u8"]
    assert np.array_equal(got, ref.apply_plan(x, plan))
    name, H0, W0, crop, size, seed = CASES[4]
    fr = torch.from_numpy(frame(H0, W0, seed)).cuda()
    pre = FramePreprocessor(crop, size)
    with hip.LaunchRecorder() as rec:
        pre(fr, augment=AUG, plan=AugmentPlan.from_slots([MIXED[3]], *size))
    assert [fn.__name__ for fn, _ in rec.calls] == ["pmoe_resample_u8_horizontal", "pmoe_resample_u8_vertical_to_u8",
                                                    "pmoe_augment_point_to_f32"]
    with hip.LaunchRecorder() as rec:
        pre(fr, augment=AUG, plan=AugmentPlan.from_slots([MIXED[1]], *size))
    assert len(rec.calls) == 6
    with hip.LaunchRecorder() as rec:
        pre(fr)
    assert [fn.__name__ for fn, _ in rec.calls] == ["pmoe_resample_u8_horizontal", "pmoe_resample_u8_vertical_to_f32"]


def test_empty_plan_is_todays_pipeline_bit_for_bit(golden_dir):
    name, H0, W0, crop, size, seed = CASES[0]
    fr = torch.from_numpy(frame(H0, W0, seed)).cuda()
    pre = FramePreprocessor(crop, size)
    plain = pre(fr)
    g = np.load(golden_dir / "prep.npz")
    assert torch.equal(plain.cpu(), torch.from_numpy(ref.to_tensor(g[name][None])[0]))
    out = pre(fr, augment=AUG, plan=AugmentPlan.empty(1, *size))
    assert out.dtype == torch.float32 and out.shape == plain.shape and torch.equal(out, plain)
    off = get_augmenter(64000, 64, "super_hard")
    for o in off.ops:
        o["freq"] = 0.0
    assert torch.equal(pre(fr, augment=off), plain)
    assert torch.equal(off(torch.from_numpy(g[name]).cuda()).cpu(), torch.from_numpy(g[name]))


def test_full_pipeline_equals_totensor_of_the_reference_on_the_pillow_fixture(golden_dir):
    name, H0, W0, crop, size, seed = CASES[4]                                # odd 97 x 65 output
    g = np.load(golden_dir / "prep.npz")
    fr = torch.from_numpy(frame(H0, W0, seed)).cuda()
    batch = torch.stack([fr, fr, fr, fr])
    plan = AugmentPlan.from_slots(MIXED, *size)
    want = ref.to_tensor(ref.apply_plan(np.stack([g[name]] * 4), plan))
    got = FramePreprocessor(crop, size)(batch, augment=AUG, plan=plan)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want))


def test_batched_leading_dims_keep_their_shape_and_frame_i_uses_row_i(golden_dir):
    name, H0, W0, crop, size, seed = CASES[3]
    one = torch.from_numpy(frame(H0, W0, seed)).cuda()
    batch = torch.stack([torch.stack([one, one, one]), torch.stack([one, one, one])])      # [2, 3, H0, W0, 3]
    slots = [[{"op": "add", "p": 10 * i}] for i in range(6)]
    plan = AugmentPlan.from_slots(slots, *size)
    pre = FramePreprocessor(crop, size)
    out = pre(batch, augment=AUG, plan=plan)
    assert out.shape == (2, 3, 3) + tuple(size)
    res = g = np.load(golden_dir / "prep.npz")[name]
    for i in range(6):
        want = ref.to_tensor(ref.op_add(res.astype(np.int64), 10 * i).astype(np.uint8)[None])[0]
        assert torch.equal(out[i // 3, i % 3].cpu(), torch.from_numpy(want)), i
    u8 = torch.from_numpy(g).cuda()
    both = AUG(torch.stack([torch.stack([u8, u8, u8]), torch.stack([u8, u8, u8])]), plan=plan)
    assert both.shape == (2, 3) + g.shape and both.dtype == torch.uint8
    assert torch.equal(both[1, 2].cpu(), torch.from_numpy(ref.op_add(g.astype(np.int64), 50).astype(np.uint8)))
    with pytest.raises(ValueError):
        pre(batch[0], augment=AUG, plan=plan)                                # 3 frames, 6 rows


def test_determinism():
    x = torch.from_numpy(_frames(8, 32, 32, seed=7)).cuda()
    aug = get_augmenter(aug_type="segmentation")
    for o in aug.ops:
        o["freq"] = 0.9
    plan = aug.plan(8, 32, 32, generator=torch.Generator().manual_seed(3))
    assert plan.has_blur and int(plan.n_slots.sum()) > 8
    assert torch.equal(aug(x, plan=plan), aug(x, plan=plan))
    a = aug(x, generator=torch.Generator().manual_seed(5))
    b = aug(x, generator=torch.Generator().manual_seed(5))
    c = aug(x, generator=torch.Generator().manual_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, x)


def test_gaussian_noise_moments():
    n, h, w, scale = 3, 64, 64, 20.0
    x = np.full((n, h, w, 3), 128, dtype=np.uint8)
    for pc in (0, 1):
        plan = AugmentPlan.from_slots([[{"op": "noise", "p": scale, "per_channel": pc, "seed": 1000 + i}] for i in range(n)], h, w)
        out = _run(x, plan).astype(np.float64)
        assert out.min() > 0 and out.max() < 255                             # 6.4 sigma: the clamp never acts
        equal = (out[..., 0] == out[..., 1]) & (out[..., 1] == out[..., 2])
        if pc:
            assert not equal.all()
            d = out - 128
        else:
            assert equal.all()
            d = out[..., 0] - 128                                            # the independent values
        N = d.size
        print(f"noise per_channel={pc}: N={N} mean={d.mean():.4f} std={d.std():.4f}")
        assert abs(d.mean()) <= 5 * scale / math.sqrt(N)
        assert abs(d.std() - math.sqrt(scale * scale + 1 / 12)) <= 5 * scale / math.sqrt(2 * N)
        # loose agreement with the numpy restatement (log / cos differ in the last bit: a value may round the other way)
        want = ref.apply_plan(x, plan).astype(np.float64)
        assert np.abs(out - want).max() <= 1 and (out != want).mean() < 0.01
    ident = AugmentPlan.from_slots([[{"op": "noise", "p": 0.0, "per_channel": 1, "seed": 4}]] * n, h, w)
    y = _frames(n, h, w, seed=8)
    assert np.array_equal(_run(y, ident), y)
