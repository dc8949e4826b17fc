"""Train-time image augmenter on the device: the ``Augment(get_augmenter(iteration, aug_type, bsz))`` step that the reference's
training path puts between ``Resize`` and ``ToTensor`` (``model/data_loader.py:255-271``, ``:88-96``; ``model/augmenter.py``).

What is the reference's: the ``get_augmenter`` surface and its eight ``aug_type`` names, the operator set of each type, the
schedule formulas, the ``Sometimes`` probabilities, the parameter ranges, ``random_order=True``.

What is NOT claimed: parity with imgaug's random stream or with its cv2 / numpy arithmetic.  imgaug is not a dependency of this
project and nothing here was compared against it.  The contract is instead:

* randomness comes from torch's CPU generator (the per-frame *plan*: which operators, in which order, with which parameters and
  seeds) and from the project's counter hash ``hash_uniform`` (per-pixel masks and noise, ``csrc/common.h``);
* each operator's arithmetic is defined in ``include/pmoe_hip.h`` (integer or single f32 operations, round-half-even, clamp to
  [0, 255]; the blur is two integer passes with 16-bit fixed-point taps and reflect-101 borders) and is restated in numpy by
  ``tests/augment_ref.py``; the device result equals that restatement bit for bit for every operator but the Gaussian noise
  (whose ``logf`` / ``cosf`` are the device's);
* the output is a pure function of (pixels, plan).

``Augmenter.plan`` draws a plan on the host; the kernels (``csrc/augment.hip``) take nothing but pixels and the plan, which goes
up in one pinned, non-blocking copy on the current stream.  There is no CPU path.
"""
import ctypes as C
import math

import torch

from .hip import check, load, stream_ptr

OP_NONE, OP_ADD, OP_MULTIPLY, OP_CONTRAST, OP_GRAYSCALE, OP_DROPOUT, OP_COARSE_DROPOUT, OP_NOISE, OP_BLUR = range(9)   # PMOE_AUG_*
OP_NAMES = ("none", "add", "multiply", "contrast", "grayscale", "dropout", "coarse_dropout", "noise", "blur")
MAX_SLOTS, MAX_TAPS = 8, 33                     # PMOE_AUG_MAX_SLOTS, PMOE_AUG_MAX_TAPS
GRAY_COEFFS = (4899, 9617, 1868)                # 0.299, 0.587, 0.114 in 14-bit fixed point (sum 16384)
PLAN_WORDS = 118                                # sizeof(pmoe_aug_plan) / 4
_SLOT0, _SLOT_WORDS, _TAPS0 = 4, 10, 4 + 8 * 10  # word offsets inside a pmoe_aug_plan row
_PER_CHANNEL_PARAM = (OP_ADD, OP_MULTIPLY, OP_CONTRAST)             # per_channel: one parameter draw per channel
_PER_CHANNEL_MASK = (OP_DROPOUT, OP_COARSE_DROPOUT, OP_NOISE)       # per_channel: one mask / noise draw per channel value
AUG_TYPES = ("medium", "soft", "high", "medium_harder", "super_hard", "custom", "soft_harder", "segmentation")


def blur_kernel_size(sigma):
    """Tap count of a blur with this sigma: ``K0 = 3.3 sigma`` below 3, ``2.9 sigma`` below 5, else ``2.6 sigma``;
    ``K = max(5, int(K0))``, plus 1 if even."""
    k0 = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = max(5, int(k0))
    return k + 1 if k % 2 == 0 else k


def blur_taps(sigma, h=None, w=None):
    """-> list of K integers: Gaussian weights in float64, normalised, ``floor(w * 65536 + 0.5)``, the centre tap corrected so
    that they sum to 65536.  ``ValueError`` for K > 33 or (given the frame size) K // 2 >= min(h, w)."""
    k = blur_kernel_size(sigma)
    if k > MAX_TAPS:
        raise ValueError(f"augment: blur sigma {sigma:g} needs {k} taps, the kernels take at most {MAX_TAPS}")
    if h is not None and k // 2 >= min(h, w):
        raise ValueError(f"augment: a {k}-tap blur (sigma {sigma:g}) does not fit a {h} x {w} frame (reflect-101 needs K // 2 < min(h, w))")
    r = k // 2
    g = [math.exp(-0.5 * ((i - r) / sigma) ** 2) for i in range(k)]
    s = sum(g)
    q = [int(math.floor(v / s * 65536.0 + 0.5)) for v in g]
    q[r] += 65536 - sum(q)
    return q


class AugmentPlan:
    """What the kernels read besides pixels, as CPU tensors (``n`` frames, up to 8 slots each, in execution order):

    ``n_slots [n]`` int32, ``ops [n, 8]`` int32 (``OP_*``), ``params [n, 8, 3]`` float32 (per channel; equal when the operator is
    not per-channel; ADD holds integers; mask and noise operators read channel 0), ``per_channel [n, 8]`` int32 (mask / noise
    operators), ``mask_hw [n, 8, 2]`` int32 (COARSE_DROPOUT's low-resolution size), ``seeds [n, 8]`` int64, ``blur_slot [n]``
    int32 (-1: none), ``blur_k [n]`` int32, ``taps [n, 33]`` int32.  ``h, w`` is the frame size the plan was made for.

    Build one by hand with ``AugmentPlan.from_slots``; ``Augmenter.plan`` draws one."""

    def __init__(self, n, h, w):
        self.n, self.h, self.w = int(n), int(h), int(w)
        self.n_slots = torch.zeros(n, dtype=torch.int32)
        self.ops = torch.zeros(n, MAX_SLOTS, dtype=torch.int32)
        self.params = torch.zeros(n, MAX_SLOTS, 3, dtype=torch.float32)
        self.per_channel = torch.zeros(n, MAX_SLOTS, dtype=torch.int32)
        self.mask_hw = torch.zeros(n, MAX_SLOTS, 2, dtype=torch.int32)
        self.seeds = torch.zeros(n, MAX_SLOTS, dtype=torch.int64)
        self.blur_slot = torch.full((n,), -1, dtype=torch.int32)
        self.blur_k = torch.zeros(n, dtype=torch.int32)
        self.taps = torch.zeros(n, MAX_TAPS, dtype=torch.int32)

    @classmethod
    def empty(cls, n, h, w):
        """no operator on any frame"""
        return cls(n, h, w)

    @classmethod
    def from_slots(cls, frames, h, w):
        """``frames``: per frame a list of slots in execution order, each a dict with ``op`` (an ``OP_*`` code or its name) and,
        as the operator needs them, ``p`` (a number or three), ``per_channel``, ``hl``, ``wl``, ``seed``, ``sigma`` (blur)."""
        plan = cls(len(frames), h, w)
        for i, slots in enumerate(frames):
            if len(slots) > MAX_SLOTS:
                raise ValueError(f"augment: a frame takes at most {MAX_SLOTS} slots")
            for s, d in enumerate(slots):
                op = OP_NAMES.index(d["op"]) if isinstance(d["op"], str) else int(d["op"])
                plan.ops[i, s] = op
                if op == OP_BLUR:
                    if plan.blur_slot[i] >= 0:
                        raise ValueError("augment: one blur per frame")
                    q = blur_taps(float(d["sigma"]), h, w)
                    plan.blur_slot[i], plan.blur_k[i] = s, len(q)
                    plan.taps[i, :len(q)] = torch.tensor(q, dtype=torch.int32)
                    plan.params[i, s] = float(d["sigma"])
                    continue
                p = d.get("p", 0.0)
                plan.params[i, s] = torch.tensor(list(p) if isinstance(p, (tuple, list)) else [p] * 3, dtype=torch.float32)
                plan.per_channel[i, s] = int(bool(d.get("per_channel", 0)))
                if op == OP_COARSE_DROPOUT:
                    plan.mask_hw[i, s, 0], plan.mask_hw[i, s, 1] = int(d["hl"]), int(d["wl"])
                plan.seeds[i, s] = int(d.get("seed", 0))
            plan.n_slots[i] = len(slots)
        return plan

    @property
    def has_blur(self):
        return bool((self.blur_slot >= 0).any())

    def packed(self, pin=False):
        """-> int32 ``[n, 118]``: one ``pmoe_aug_plan`` row per frame (include/pmoe_hip.h)"""
        n = self.n
        row = torch.zeros(n, PLAN_WORDS, dtype=torch.int32, pin_memory=pin)
        row[:, 0], row[:, 1], row[:, 2] = self.n_slots, self.blur_slot, self.blur_k
        slots = row[:, _SLOT0:_TAPS0].view(n, MAX_SLOTS, _SLOT_WORDS)
        slots[:, :, 0], slots[:, :, 1] = self.ops, self.per_channel
        slots[:, :, 2:4] = self.mask_hw
        slots[:, :, 4:7] = self.params.contiguous().view(torch.int32)
        slots[:, :, 8:10] = self.seeds.contiguous().view(torch.int32).view(n, MAX_SLOTS, 2)      # little endian: low word first
        row[:, _TAPS0:_TAPS0 + MAX_TAPS] = self.taps
        return row


def _clamp01(v):
    return min(max(float(v), 0.0), 1.0)


class Augmenter:
    """A cheap host object (no device state): ``ops`` is the reference's ``iaa.Sequential`` list for one ``aug_type`` at one
    ``iteration`` -- per operator its ``Sometimes`` probability, parameter range and ``per_channel`` probability -- and
    ``factors`` the schedule values it was built from."""

    def __init__(self, aug_type, factors, ops):
        self.aug_type, self.factors, self.ops = aug_type, factors, ops

    # ---- the plan: every draw is a torch.rand / torch.randint call with `generator`, vectorised over the n frames
    def plan(self, n, h, w, generator=None):
        """Draw order (fixed: it is the stream contract): selection ``rand [n, M]``, order keys ``rand [n, M]``, per-channel
        ``rand [n, M]``, parameters ``rand [n, M, 3]`` (float64), ``Add`` values ``randint [n, 3]``, mask sizes ``rand [n, M]``,
        seeds ``randint [n, M]`` -- all of them always, whatever the earlier draws selected."""
        n, h, w = int(n), int(h), int(w)
        M = len(self.ops)
        plan = AugmentPlan(n, h, w)
        if n < 1 or M == 0:
            return plan
        g = generator
        freq = torch.tensor([_clamp01(o["freq"]) for o in self.ops], dtype=torch.float64)
        pc_prob = torch.tensor([_clamp01(o.get("per_channel", 0.0)) for o in self.ops], dtype=torch.float64)
        sel = torch.rand(n, M, generator=g, dtype=torch.float64) < freq                # Sometimes(f, op): Bernoulli(f) per frame and op
        keys = torch.rand(n, M, generator=g, dtype=torch.float64)                      # random_order: a uniform permutation per frame
        pc = torch.rand(n, M, generator=g, dtype=torch.float64) < pc_prob              # float per_channel=c: Bernoulli(c) per frame
        u = torch.rand(n, M, 3, generator=g, dtype=torch.float64)
        add_op = next((o for o in self.ops if o["op"] == OP_ADD), None)
        fa = int(math.floor(add_op["range"][1])) if add_op is not None else 0
        add_val = torch.randint(-fa, fa + 1, (n, 3), generator=g)                      # integer uniform in [-floor(a), floor(a)]
        usize = torch.rand(n, M, generator=g, dtype=torch.float64)
        seeds = torch.randint(0, 2 ** 63 - 1, (n, M), generator=g, dtype=torch.int64)

        codes = torch.tensor([o["op"] for o in self.ops], dtype=torch.int32)
        lo = torch.tensor([o["range"][0] for o in self.ops], dtype=torch.float64)
        hi = torch.tensor([o["range"][1] for o in self.ops], dtype=torch.float64)
        val = lo[None, :, None] + (hi - lo)[None, :, None] * u                          # uniform in the range, per channel
        for m, o in enumerate(self.ops):
            if o["op"] == OP_ADD:
                val[:, m] = add_val.to(torch.float64)
        per_param = torch.tensor([o["op"] in _PER_CHANNEL_PARAM for o in self.ops])
        spread = (pc & per_param)[:, :, None]
        val = torch.where(spread, val, val[:, :, :1].expand(-1, -1, 3))                # not per-channel: channel 0's draw for all
        mask_pc = pc & torch.tensor([o["op"] in _PER_CHANNEL_MASK for o in self.ops])
        mask_hw = torch.zeros(n, M, 2, dtype=torch.int32)
        for m, o in enumerate(self.ops):
            if o["op"] == OP_COARSE_DROPOUT:
                s = o["size_percent"][0] + (o["size_percent"][1] - o["size_percent"][0]) * usize[:, m]
                mask_hw[:, m, 0] = torch.clamp(torch.floor(h * s), min=3).clamp(max=h).to(torch.int32)
                mask_hw[:, m, 1] = torch.clamp(torch.floor(w * s), min=3).clamp(max=w).to(torch.int32)
            if o["op"] == OP_BLUR:
                sel[:, m] &= val[:, m, 0] >= 1e-3                                      # a blur below 1e-3 is the identity: skipped
        # execution order: the selected operators by their order key
        order = torch.where(sel, keys, keys + 2.0).argsort(dim=1)
        count = sel.sum(dim=1)
        k = min(M, MAX_SLOTS)
        live = torch.arange(k)[None, :] < count[:, None]
        idx = order[:, :k]
        plan.n_slots = count.to(torch.int32)
        plan.ops[:, :k] = torch.where(live, codes[idx], torch.zeros((), dtype=torch.int32))
        plan.params[:, :k] = torch.where(live[:, :, None], val.gather(1, idx[:, :, None].expand(-1, -1, 3)), 0.0).to(torch.float32)
        plan.per_channel[:, :k] = torch.where(live, mask_pc.gather(1, idx), False).to(torch.int32)
        plan.mask_hw[:, :k] = torch.where(live[:, :, None], mask_hw.gather(1, idx[:, :, None].expand(-1, -1, 2)), 0)
        plan.seeds[:, :k] = torch.where(live, seeds.gather(1, idx), 0)
        is_blur = plan.ops == OP_BLUR
        for i in torch.nonzero(is_blur.any(dim=1)).flatten().tolist():                 # the taps: float64 host arithmetic per blurred frame
            s = int(is_blur[i].to(torch.int32).argmax())
            q = blur_taps(float(plan.params[i, s, 0]), h, w)
            plan.blur_slot[i], plan.blur_k[i] = s, len(q)
            plan.taps[i, :len(q)] = torch.tensor(q, dtype=torch.int32)
        return plan

    # ---- the stand-alone form of seq.augment_images
    def __call__(self, images_u8, generator=None, plan=None):
        """uint8 device ``[..., h, w, 3]`` -> the same shape and dtype, augmented (frame i of the flattened batch by plan row i)"""
        _check_frames(images_u8, "Augmenter")
        h, w = images_u8.shape[-3:-1]
        src = images_u8.contiguous().view(-1, h, w, 3)
        plan = self._plan_for(src.shape[0], h, w, generator, plan)
        out = torch.empty_like(src)
        run_plan(src, plan, out)
        return out.view(images_u8.shape)

    def _plan_for(self, n, h, w, generator, plan):
        if plan is None:
            return self.plan(n, h, w, generator)
        if not isinstance(plan, AugmentPlan):
            raise TypeError("augment: plan must be an AugmentPlan")
        if (plan.n, plan.h, plan.w) != (n, h, w):
            raise ValueError(f"augment: the plan is for {plan.n} frames of {plan.h} x {plan.w}, got {n} frames of {h} x {w}")
        return plan


def _check_frames(t, who):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError(f"{who}: expected a uint8 tensor [..., h, w, 3]")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: frames must be on the MI355X (cuda) device; pmoe_amd has no CPU path")
    if t.dim() < 3 or t.shape[-1] != 3:
        raise ValueError(f"{who}: expected [..., h, w, 3]")


def run_plan(src, plan, out):
    """``src`` uint8 ``[n, h, w, 3]`` on the device (left unchanged), ``out`` uint8 ``[n, h, w, 3]`` or float32 ``[n, 3, h, w]``
    (``value / 255``: ToTensor).  Launches: point phase 0, and when some frame of the plan has a blur: blur H, blur V, point
    phase 1.  No host synchronisation; the plan goes up in one pinned non-blocking copy on the current stream."""
    n, h, w, _ = src.shape
    k = int(plan.blur_k.max()) if plan.n else 0
    if k > MAX_TAPS or (k and k // 2 >= min(h, w)):
        raise ValueError(f"augment: a {k}-tap blur does not fit a {h} x {w} frame / the kernels' {MAX_TAPS} taps")
    if int(plan.n_slots.max()) > MAX_SLOTS or int(plan.n_slots.min()) < 0:
        raise ValueError(f"augment: n_slots must be 0..{MAX_SLOTS}")
    dev = src.device
    rows = plan.packed(pin=True).to(dev, non_blocking=True)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    lib = load()
    last = lib.pmoe_augment_point_to_f32 if out.dtype == torch.float32 else lib.pmoe_augment_point_to_u8
    if not plan.has_blur:
        check(last(p(src), p(out), p(rows), n, h, w, 0, stream_ptr()), "pmoe_augment_point")
        return out
    a, b = torch.empty_like(src), torch.empty_like(src)
    check(lib.pmoe_augment_point_to_u8(p(src), p(a), p(rows), n, h, w, 0, stream_ptr()), "pmoe_augment_point_to_u8")
    check(lib.pmoe_augment_blur_h(p(a), p(b), p(rows), n, h, w, stream_ptr()), "pmoe_augment_blur_h")
    check(lib.pmoe_augment_blur_v(p(b), p(a), p(rows), n, h, w, stream_ptr()), "pmoe_augment_blur_v")
    check(last(p(a), p(out), p(rows), n, h, w, 1, stream_ptr()), "pmoe_augment_point")
    return out


# ---- the schedules of model/augmenter.py, per type.  Each returns the nine factors the reference prints under DEBUG
# (frequency, color, dropout, blur, add, multiply +/-, contrast +/-); None where the type has no such operator.
_SCHEDULES = {   # type: (iteration divisor of bsz, freq / color denominators, blur, add, multiply (pos, neg), contrast (pos, neg))
    "medium": (1.5, 1000000.0, 1000000.0, 100000.0, 150000.0, (500000.0, 500000.0), (500000.0, 500000.0)),         # :79-95
    "soft": (1.5, 1200000.0, 1200000.0, 120000.0, 170000.0, (800000.0, 800000.0), (800000.0, 800000.0)),            # :157-173
    "high": (1.5, 800000.0, 800000.0, 80000.0, 120000.0, (350000.0, 400000.0), (350000.0, 400000.0)),               # :235-251
    "medium_harder": (1.0, 1000000.0, 1000000.0, 100000.0, 150000.0, (500000.0, 500000.0), (500000.0, 500000.0)),  # :313-329
    "super_hard": (1.0, 50000.0, 100000.0, 100000.0, 100000.0, (200000.0, 500000.0), (500000.0, 500000.0)),         # :391-411
    "soft_harder": (1.0, 1200000.0, 1200000.0, 120000.0, 170000.0, (800000.0, 800000.0), (800000.0, 800000.0)),     # :537-553
}


def schedule(aug_type, image_iteration=1, bsz=32):
    """-> dict of the nine schedule factors of ``model/augmenter.py`` for this type (unclamped, as the reference computes them)"""
    if aug_type == "segmentation":                                  # seg_aug(): no schedule
        return dict.fromkeys(("frequency_factor", "color_factor", "dropout_factor", "blur_factor", "add_factor",
                              "multiply_factor_pos", "multiply_factor_neg", "contrast_factor_pos", "contrast_factor_neg"))
    if aug_type == "custom":                                        # :473-485: only four factors, the rest are constants in its list
        iteration = image_iteration / bsz
        return {"frequency_factor": min(0.05 + float(iteration) / 50000.0, 1.0), "color_factor": float(iteration) / 100000.0,
                "dropout_factor": 0.198667 + (0.03856658 - 0.198667) / (1 + (iteration / 196416.6) ** 1.863486),
                "blur_factor": 0.5 + (0.5 * iteration / 20000.0), "add_factor": None, "multiply_factor_pos": None,
                "multiply_factor_neg": None, "contrast_factor_pos": None, "contrast_factor_neg": None}
    div, fden, cden, bden, aden, (mpos, mneg), (cpos, cneg) = _SCHEDULES[aug_type]
    iteration = image_iteration / (bsz * div)
    freq = 0.05 + float(iteration) / fden
    if aug_type == "super_hard":
        freq = min(freq, 1.0)
    return {"frequency_factor": freq, "color_factor": float(iteration) / cden,
            "dropout_factor": 0.198667 + (0.03856658 - 0.198667) / (1 + (iteration / 196416.6) ** 1.863486),
            "blur_factor": 0.5 + (0.5 * iteration / bden), "add_factor": 10 + 10 * iteration / aden,
            "multiply_factor_pos": 1 + (2.5 * iteration / mpos), "multiply_factor_neg": 1 - (0.91 * iteration / mneg),
            "contrast_factor_pos": 1 + (0.5 * iteration / cpos), "contrast_factor_neg": 1 - (0.5 * iteration / cneg)}


def _op(op, freq, rng, per_channel=0.0, **kw):
    return dict(op=op, freq=_clamp01(freq), range=(float(rng[0]), float(rng[1])), per_channel=_clamp01(per_channel), **kw)


def get_augmenter(iteration=1, bsz=32, aug_type="medium"):
    """``model/augmenter.py:17-40``: same signature, names and error.  Probabilities are clamped to [0, 1] (``super_hard``'s
    ``color_factor`` exceeds 1 late in training)."""
    if aug_type not in AUG_TYPES:
        raise ValueError(
            "Unknown augmentation, value should be one of"
            "'medium', 'high', 'medium_harder', 'super_hard', 'soft_harder', 'custom'"
        )
    if aug_type == "segmentation":
        # seg_aug() (:57-76) leaves these ranges to imgaug's defaults.  They are imgaug 0.4.0's DOCUMENTED defaults, taken from
        # its documentation and unpinned (imgaug is not installed where this was written): GaussianBlur sigma (0, 3.0),
        # AdditiveGaussianNoise scale (0, 15), CoarseDropout p (0.02, 0.1), Dropout p (0, 0.05), LinearContrast alpha (0.6, 1.4)
        ops = [_op(OP_BLUR, 0.3, (0.0, 3.0)),
               _op(OP_NOISE, 0.3, (0.0, 15.0), 1.0),
               _op(OP_COARSE_DROPOUT, 0.1, (0.02, 0.1), 1.0, size_percent=(0.08, 0.2)),
               _op(OP_DROPOUT, 0.1, (0.0, 0.05), 1.0),
               _op(OP_CONTRAST, 0.2, (0.6, 1.4), 1.0)]
        return Augmenter(aug_type, schedule(aug_type), ops)
    f = schedule(aug_type, iteration, bsz)
    fr, col, drop = f["frequency_factor"], f["color_factor"], f["dropout_factor"]
    ops = [_op(OP_BLUR, fr, (0.0, f["blur_factor"])),
           _op(OP_NOISE, fr, (0.0, drop), col)]
    if aug_type != "custom":
        ops.append(_op(OP_COARSE_DROPOUT, fr, (0.0, drop), col, size_percent=(0.08, 0.2)))
    ops.append(_op(OP_DROPOUT, fr, (0.0, drop), col))
    if aug_type == "custom":                                        # :522-524
        ops += [_op(OP_ADD, fr, (-30.0, 30.0), 0.0), _op(OP_MULTIPLY, fr, (0.9, 1.3), 1.0)]
    else:
        ops += [_op(OP_ADD, fr, (-f["add_factor"], f["add_factor"]), col),
                _op(OP_MULTIPLY, fr, (f["multiply_factor_neg"], f["multiply_factor_pos"]), col),
                _op(OP_CONTRAST, fr, (f["contrast_factor_neg"], f["contrast_factor_pos"]), col)]
        if aug_type != "super_hard":                                # :465: super_hard comments the grayscale out
            ops.append(_op(OP_GRAYSCALE, fr, (0.0, 1.0)))
    return Augmenter(aug_type, f, ops)
