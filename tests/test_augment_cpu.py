"""Host side of the train-time augmenter (pmoe_amd/augment.py): the reference's schedules, the blur taps, the plan's statistics
and the numpy restatement (tests/augment_ref.py) against an independent yardstick.  No GPU."""
import math

import numpy as np
import pytest
import torch

from pmoe_amd import augment
from pmoe_amd.augment import AugmentPlan, blur_kernel_size, blur_taps, get_augmenter, schedule
from tests import augment_ref as ref

FACTORS = ("frequency_factor", "color_factor", "dropout_factor", "blur_factor", "add_factor", "multiply_factor_pos",
           "multiply_factor_neg", "contrast_factor_pos", "contrast_factor_neg")
D0 = 0.03856658                 # dropout_factor at iteration 0: 0.198667 + (0.03856658 - 0.198667) / (1 + 0)
# dropout_factor at iteration = 196416.6 (the curve's midpoint: (1)**1.863486 = 1): 0.198667 + (0.03856658 - 0.198667) / 2
DMID = 0.11861679
# Written out by hand from the formulas of model/augmenter.py (the lines cited per type).  Two points each: image_iteration = 0,
# and the image_iteration that makes the reference's `iteration` equal 196416.6 (bsz = 32: 196416.6 * 32 * 1.5 = 9427996.8 for
# the types that divide by bsz * 1.5, 196416.6 * 32 = 6285331.2 for those that divide by bsz).
I15, I10 = 9427996.8, 6285331.2
X = 196416.6
SCHEDULES = {
    # medium (:79-95): iteration = i / (bsz * 1.5); 0.05 + it / 1e6; it / 1e6; blur 0.5 + 0.5 it / 1e5; add 10 + 10 it / 1.5e5;
    # multiply 1 + 2.5 it / 5e5, 1 - 0.91 it / 5e5; contrast 1 +- 0.5 it / 5e5
    "medium": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
               (I15, (0.05 + 0.1964166, 0.1964166, DMID, 0.5 + 0.982083, 10 + 13.09444, 1 + 0.982083, 1 - 0.357478212,
                      1 + 0.1964166, 1 - 0.1964166))],
    # soft (:157-173): 1.2e6, 1.2e6, blur / 1.2e5, add / 1.7e5, multiply / 8e5, contrast / 8e5
    "soft": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
             (I15, (0.05 + 0.1636805, 0.1636805, DMID, 0.5 + 0.81840250, 10 + 11.553918, 1 + 0.613801875, 1 - 0.2234238825,
                    1 + 0.122760375, 1 - 0.122760375))],
    # high (:235-251): 8e5, 8e5, blur / 8e4, add / 1.2e5, multiply + / 3.5e5, - / 4e5, contrast + / 3.5e5, - / 4e5
    "high": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
             (I15, (0.05 + 0.24552075, 0.24552075, DMID, 0.5 + 1.22760375, 10 + 16.36805, 1 + 1.402975714, 1 - 0.446847765,
                    1 + 0.280595143, 1 - 0.24552075))],
    # medium_harder (:313-329): iteration = i / bsz, then medium's constants
    "medium_harder": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
                      (I10, (0.05 + 0.1964166, 0.1964166, DMID, 0.5 + 0.982083, 10 + 13.09444, 1 + 0.982083, 1 - 0.357478212,
                             1 + 0.1964166, 1 - 0.1964166))],
    # super_hard (:391-411): i / bsz; min(0.05 + it / 5e4, 1); it / 1e5; blur / 1e5; add / 1e5; multiply + / 2e5, - / 5e5;
    # contrast / 5e5
    "super_hard": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
                   (I10, (1.0, 1.964166, DMID, 0.5 + 0.982083, 10 + 19.64166, 1 + 2.4552075, 1 - 0.357478212,
                          1 + 0.1964166, 1 - 0.1964166))],
    # custom (:473-485): i / bsz; min(0.05 + it / 5e4, 1); it / 1e5; blur 0.5 + 0.5 it / 2e4; the rest are constants of its list
    "custom": [(0, (0.05, 0.0, D0, 0.5, None, None, None, None, None)),
               (I10, (1.0, 1.964166, DMID, 0.5 + 4.910415, None, None, None, None, None))],
    # soft_harder (:537-553): i / bsz, then soft's constants
    "soft_harder": [(0, (0.05, 0.0, D0, 0.5, 10.0, 1.0, 1.0, 1.0, 1.0)),
                    (I10, (0.05 + 0.1636805, 0.1636805, DMID, 0.5 + 0.81840250, 10 + 11.553918, 1 + 0.613801875,
                           1 - 0.2234238825, 1 + 0.122760375, 1 - 0.122760375))],
    # segmentation (:57-76): seg_aug() has no schedule
    "segmentation": [(0, (None,) * 9), (I10, (None,) * 9)],
}


@pytest.mark.parametrize("aug_type", augment.AUG_TYPES)
def test_schedules_are_the_references(aug_type):
    assert set(SCHEDULES) == set(augment.AUG_TYPES)
    for it, want in SCHEDULES[aug_type]:
        got = schedule(aug_type, it, 32)
        assert tuple(got) == FACTORS
        for name, w in zip(FACTORS, want):
            if w is None:
                assert got[name] is None, (aug_type, name)
            else:
                assert got[name] == pytest.approx(w, rel=2e-6, abs=1e-9), (aug_type, it, name)
        assert get_augmenter(it, 32, aug_type).factors == got


def test_operator_lists_are_the_references():
    """operator set, Sometimes probability, ranges and per_channel of each type's iaa.Sequential list, probabilities clamped"""
    def table(aug):
        return {augment.OP_NAMES[o["op"]]: o for o in aug.ops}
    full = {"blur", "noise", "coarse_dropout", "dropout", "add", "multiply", "contrast", "grayscale"}
    for t in ("medium", "soft", "high", "medium_harder", "soft_harder"):
        assert set(table(get_augmenter(1000, 32, t))) == full
    assert set(table(get_augmenter(1000, 32, "super_hard"))) == full - {"grayscale"}                     # :465 commented out
    assert set(table(get_augmenter(1000, 32, "custom"))) == {"blur", "noise", "dropout", "add", "multiply"}
    seg = table(get_augmenter(aug_type="segmentation"))
    assert {k: (v["freq"], v["range"], v["per_channel"]) for k, v in seg.items()} == {
        "blur": (0.3, (0.0, 3.0), 0.0), "noise": (0.3, (0.0, 15.0), 1.0), "coarse_dropout": (0.1, (0.02, 0.1), 1.0),
        "dropout": (0.1, (0.0, 0.05), 1.0), "contrast": (0.2, (0.6, 1.4), 1.0)}
    assert seg["coarse_dropout"]["size_percent"] == (0.08, 0.2)
    assert get_augmenter(5, 7, "segmentation").ops == get_augmenter(aug_type="segmentation").ops          # ignores both
    m = table(get_augmenter(I15, 32, "medium"))
    f = schedule("medium", I15, 32)
    assert all(o["freq"] == f["frequency_factor"] for o in m.values())
    assert m["add"]["range"] == (-f["add_factor"], f["add_factor"]) and m["add"]["per_channel"] == f["color_factor"]
    assert m["multiply"]["range"] == (f["multiply_factor_neg"], f["multiply_factor_pos"])
    assert m["contrast"]["range"] == (f["contrast_factor_neg"], f["contrast_factor_pos"])
    assert m["noise"]["range"] == m["dropout"]["range"] == m["coarse_dropout"]["range"] == (0.0, f["dropout_factor"])
    assert m["blur"]["range"] == (0.0, f["blur_factor"]) and m["grayscale"]["range"] == (0.0, 1.0)
    assert m["grayscale"]["per_channel"] == m["blur"]["per_channel"] == 0.0
    c = table(get_augmenter(64000, 64, "custom"))
    assert c["add"]["range"] == (-30.0, 30.0) and c["add"]["per_channel"] == 0.0                          # :522
    assert c["multiply"]["range"] == (0.9, 1.3) and c["multiply"]["per_channel"] == 1.0                   # :524
    late = table(get_augmenter(I10, 32, "super_hard"))                                                   # color_factor 1.96
    assert late["add"]["per_channel"] == 1.0 and late["add"]["freq"] == 1.0


def test_unknown_type_raises_the_references_text():
    with pytest.raises(ValueError) as e:
        get_augmenter(1, 32, "hard")
    assert str(e.value) == ("Unknown augmentation, value should be one of"
                            "'medium', 'high', 'medium_harder', 'super_hard', 'soft_harder', 'custom'")


def test_grey_coefficients_sum_to_one():
    assert sum(augment.GRAY_COEFFS) == 16384 == sum(ref.GRAY)
    assert augment.GRAY_COEFFS == ref.GRAY


def test_taps_sum_to_65536_and_are_non_negative():
    for sigma in np.concatenate([[1.001e-3, 0.01, 0.1], np.arange(0.25, 9.01, 0.125)]):
        q = blur_taps(float(sigma))
        k = len(q)
        assert sum(q) == 65536 and min(q) >= 0 and k % 2 == 1 and 5 <= k <= 33, (sigma, q)
        assert k == blur_kernel_size(float(sigma)) and q == q[::-1]
    assert [blur_kernel_size(s) for s in (0.5, 1.8, 2.2, 2.8, 2.99, 3.0, 4.9, 5.0, 9.0)] == [5, 5, 7, 9, 9, 9, 15, 13, 23]
    with pytest.raises(ValueError):
        blur_taps(13.5)                       # 2.6 * 13.5 = 35.1 -> 35 taps
    assert len(blur_taps(13.0)) == 33         # 2.6 * 13 = 33.8 -> 33: the widest
    with pytest.raises(ValueError):
        blur_taps(2.8, 4, 40)                 # K = 9: K // 2 = 4 >= min(h, w)


def test_reference_blur_equals_scipy_correlate1d():
    """tests/augment_ref.py's blur against scipy.ndimage.correlate1d(mode="mirror") (= reflect-101) on int64 with the same taps"""
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(5)
    for (h, w), sigma in (((19, 37), 1.0), ((16, 16), 2.2), ((5, 6), 2.8), ((40, 33), 6.0)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8).astype(np.int64)
        q = np.array(blur_taps(sigma, h, w), dtype=np.int64)
        want = (correlate1d(img, q, axis=1, mode="mirror") + 32768) >> 16
        want = (correlate1d(want, q, axis=0, mode="mirror") + 32768) >> 16
        got = ref.op_blur(img, q)
        assert np.array_equal(got, want) and got.min() >= 0 and got.max() <= 255


def test_reference_hash_is_the_counter_hash():
    """splitmix64's published first outputs for seed 0 are hash(state) of 1, 2, 3 x the golden-ratio increment: the top 24 bits"""
    known = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    got = ref.hash_uniform(0, np.array([1, 2, 3]))
    assert [float(g) for g in got] == [(k >> 40) / 16777216.0 for k in known]


N, F = 4096, 0.3


def _forced(aug_type="medium", f=F, c=0.5):
    aug = get_augmenter(1000, 32, aug_type)
    for o in aug.ops:
        o["freq"], o["per_channel"] = f, (c if o["per_channel"] is not None else 0.0)
    return aug


def test_plan_statistics():
    aug = _forced()
    for o in aug.ops:                         # sigma in (0.5, 2): never below the 1e-3 skip, so blur is selected like the others
        if o["op"] == augment.OP_BLUR:
            o["range"] = (0.5, 2.0)
    M = len(aug.ops)
    g = torch.Generator().manual_seed(123)
    plan = aug.plan(N, 64, 48, generator=g)
    live = torch.arange(8)[None, :] < plan.n_slots[:, None]
    assert (plan.ops[~live] == 0).all() and (plan.ops[live] > 0).all()
    tol = 5 * math.sqrt(F * (1 - F) / N)
    for o in aug.ops:
        here = (plan.ops == o["op"]) & live
        assert (here.sum(1) <= 1).all()                                                 # each operator at most once per frame
        share = here.any(1).double().mean().item()
        assert abs(share - F) <= tol, (o["op"], share)
        # position among the selected operators: given m selected, a uniform permutation puts the operator at 0..m-1 uniformly.
        # Normalised position u = pos / (m - 1) over frames with m >= 2 has mean 1/2 and variance (m + 1) / (12 (m - 1)) <= 1/4
        # (m = 2), so the mean of u over F such frames is within 5 * sqrt(1/4 / F) of 1/2.
        rows = here.any(1) & (plan.n_slots >= 2)
        pos = here[rows].double().argmax(1)
        u = pos / (plan.n_slots[rows] - 1).double()
        assert abs(u.mean().item() - 0.5) <= 5 * math.sqrt(0.25 / int(rows.sum())), (o["op"], u.mean().item())
        lo, hi = o["range"]
        vals = plan.params[here]
        if o["op"] == augment.OP_ADD:
            assert (vals == vals.round()).all() and vals.min() >= -math.floor(hi) and vals.max() <= math.floor(hi)
            assert vals.min() == -math.floor(hi) and vals.max() == math.floor(hi)        # both ends are reachable
        else:
            assert vals.min() >= float(np.float32(lo)) and vals.max() <= float(np.float32(hi)), (o["op"], vals.min(), vals.max())
        pcs = plan.per_channel[here].double()
        differ = (vals[:, 0] != vals[:, 1]).double()
        if o["op"] in (augment.OP_DROPOUT, augment.OP_COARSE_DROPOUT, augment.OP_NOISE):
            assert abs(pcs.mean().item() - 0.5) <= 5 * math.sqrt(0.25 / len(pcs)) and differ.sum() == 0
        elif o["op"] in (augment.OP_MULTIPLY, augment.OP_CONTRAST):
            assert abs(differ.mean().item() - 0.5) <= 5 * math.sqrt(0.25 / len(differ)) and pcs.sum() == 0
        else:
            assert pcs.sum() == 0
        if o["op"] in (augment.OP_BLUR, augment.OP_GRAYSCALE):
            assert differ.sum() == 0
        if o["op"] == augment.OP_COARSE_DROPOUT:
            hw = plan.mask_hw[here]
            assert hw[:, 0].min() >= 3 and hw[:, 0].max() <= math.floor(64 * 0.2) and hw[:, 1].min() >= 3 and hw[:, 1].max() <= 9
    assert M == 8 and int(plan.n_slots.max()) <= 8
    blurred = plan.blur_slot >= 0
    assert torch.equal(blurred, ((plan.ops == augment.OP_BLUR) & live).any(1))
    k = plan.blur_k[blurred]
    assert (k % 2 == 1).all() and (k >= 5).all() and (plan.blur_k[~blurred] == 0).all()
    assert (plan.taps[blurred].sum(1) == 65536).all() and (plan.taps >= 0).all() and (plan.taps[~blurred] == 0).all()
    rows = torch.nonzero(blurred).flatten()
    assert (plan.ops[rows, plan.blur_slot[rows].long()] == augment.OP_BLUR).all()
    seeds = plan.seeds[live]
    assert seeds.min() >= 0 and len(set(seeds.tolist())) == len(seeds)


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in
               ("n_slots", "ops", "params", "per_channel", "mask_hw", "seeds", "blur_slot", "blur_k", "taps"))


def test_plan_is_reproducible_and_follows_the_default_generator():
    aug = get_augmenter(64000 * 50, 64, "super_hard")
    a = aug.plan(64, 32, 32, generator=torch.Generator().manual_seed(7))
    b = aug.plan(64, 32, 32, generator=torch.Generator().manual_seed(7))
    c = aug.plan(64, 32, 32, generator=torch.Generator().manual_seed(8))
    assert _same(a, b) and not _same(a, c)
    torch.manual_seed(7)
    d = aug.plan(64, 32, 32)
    torch.manual_seed(7)
    e = aug.plan(64, 32, 32)
    assert _same(d, e) and _same(d, a)        # a fresh Generator().manual_seed(s) is the default generator after manual_seed(s)
    assert int(a.n_slots.sum()) > 0


def test_blur_below_the_threshold_is_skipped_and_a_wide_one_is_refused():
    aug = _forced(f=1.0)
    for o in aug.ops:
        if o["op"] == augment.OP_BLUR:
            o["range"] = (0.0, 9e-4)
    plan = aug.plan(32, 16, 16, generator=torch.Generator().manual_seed(1))
    assert (plan.n_slots == 7).all() and not plan.has_blur and not (plan.ops == augment.OP_BLUR).any()
    for o in aug.ops:
        if o["op"] == augment.OP_BLUR:
            o["range"] = (4.0, 4.5)            # K = 11 or 13 on a 5 x 5 frame
    with pytest.raises(ValueError):
        aug.plan(4, 5, 5, generator=torch.Generator().manual_seed(1))


def test_packed_rows_have_the_c_layout():
    """one pmoe_aug_plan row (include/pmoe_hip.h): 4 header words, 8 slots of 10 words, 33 taps, 1 pad = 118 words"""
    plan = AugmentPlan.from_slots([[{"op": "add", "p": (1, -2, 3)}, {"op": "blur", "sigma": 1.0},
                                    {"op": "coarse_dropout", "p": 0.25, "hl": 3, "wl": 4, "per_channel": 1,
                                     "seed": 0x123456789ABCDEF}], []], 16, 16)
    rows = plan.packed()
    assert rows.shape == (2, 118) and rows.dtype == torch.int32 and augment.PLAN_WORDS * 4 == 472
    r = rows[0].tolist()
    assert r[:4] == [3, 1, 5, 0]
    assert r[4:8] == [augment.OP_ADD, 0, 0, 0] and np.array(r[8:11], dtype=np.int32).view(np.float32).tolist() == [1.0, -2.0, 3.0]
    s2 = r[4 + 20:4 + 30]
    assert s2[:4] == [augment.OP_COARSE_DROPOUT, 1, 3, 4] and np.array(s2[4:5], dtype=np.int32).view(np.float32)[0] == 0.25
    assert (s2[8] & 0xFFFFFFFF) | ((s2[9] & 0xFFFFFFFF) << 32) == 0x123456789ABCDEF
    assert r[84:89] == blur_taps(1.0) and sum(r[84:117]) == 65536 and r[117] == 0
    assert rows[1].tolist() == [0, -1, 0] + [0] * 115


def test_augmenter_rejects_cpu_and_wrong_dtypes():
    from pmoe_amd.preprocess import FramePreprocessor
    aug = get_augmenter()
    with pytest.raises(TypeError):
        aug(torch.zeros(2, 8, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        aug(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    pre = FramePreprocessor((1, 1), (8, 8))
    with pytest.raises(TypeError):
        pre(torch.zeros(12, 12, 3), augment=aug)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pre(torch.zeros(12, 12, 3, dtype=torch.uint8), augment=aug)


def test_entry_points_refuse_bad_arguments():
    """PMOE_ERR_ARG before any launch (runs without a GPU): null pointers, empty shapes, a phase other than 0 / 1, in-place u8"""
    import ctypes as C
    from pmoe_amd import hip
    lib = hip.load()
    P = C.c_void_p
    a, b, plan = P(0x1000), P(0x2000), P(0x3000)
    for fn in (lib.pmoe_augment_point_to_u8, lib.pmoe_augment_point_to_f32):
        assert fn(None, b, plan, 1, 8, 8, 0, None) == hip.ERR_ARG
        assert fn(a, None, plan, 1, 8, 8, 0, None) == hip.ERR_ARG
        assert fn(a, b, None, 1, 8, 8, 0, None) == hip.ERR_ARG
        assert fn(a, b, plan, 0, 8, 8, 0, None) == hip.ERR_ARG
        assert fn(a, b, plan, 1, 0, 8, 0, None) == hip.ERR_ARG
        assert fn(a, b, plan, 1, 8, 8, 2, None) == hip.ERR_ARG
        assert fn(a, b, plan, 65536, 8, 8, 0, None) == hip.ERR_ARG
    assert lib.pmoe_augment_point_to_u8(a, a, plan, 1, 8, 8, 0, None) == hip.ERR_ARG
    for fn in (lib.pmoe_augment_blur_h, lib.pmoe_augment_blur_v):
        assert fn(None, b, plan, 1, 8, 8, None) == hip.ERR_ARG
        assert fn(a, a, plan, 1, 8, 8, None) == hip.ERR_ARG
        assert fn(a, b, None, 1, 8, 8, None) == hip.ERR_ARG
        assert fn(a, b, plan, 1, 8, 0, None) == hip.ERR_ARG
    assert lib.pmoe_resample_u8_vertical_to_u8(a, None, 1, 8, 8, 3, 8, a, a, 3, None) == hip.ERR_ARG
    assert lib.pmoe_abi_sizeof(4) == 4 * augment.PLAN_WORDS == 472
