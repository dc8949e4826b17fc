"""numpy restatement of the train-time augmenter's operator arithmetic (pmoe_amd/augment.py, include/pmoe_hip.h), written from
the operator definitions and not from the kernels.  ``apply_plan(images_u8, plan)`` runs an ``AugmentPlan`` frame by frame.

v = a uint8 channel value as int; rint = round-half-even (np.rint); clamp to [0, 255]; every float step is ONE float32 operation
(numpy float32 arithmetic never contracts a multiply and an add).  The Gaussian noise goes through numpy's log / cos, so it
matches the device statistically, not bit for bit."""
import numpy as np

ADD, MULTIPLY, CONTRAST, GRAYSCALE, DROPOUT, COARSE_DROPOUT, NOISE, BLUR = 1, 2, 3, 4, 5, 6, 7, 8
GRAY = (4899, 9617, 1868)
f32 = np.float32


def hash_uniform(seed, idx):
    """csrc/common.h: splitmix-style counter hash -> float32 uniform in [0, 1) with 24 bits"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * f32(1.0 / 16777216.0)


def _clamp_rint(x):
    return np.clip(np.rint(x), 0, 255).astype(np.int64)


def op_add(v, k):
    return np.clip(v + np.asarray(k, dtype=np.int64), 0, 255)


def op_multiply(v, m):
    return _clamp_rint(v.astype(f32) * np.asarray(m, dtype=f32))


def op_contrast(v, a):
    return _clamp_rint(np.asarray(a, dtype=f32) * (v - 128).astype(f32) + f32(128))


def op_grayscale(v, a):
    g = (GRAY[0] * v[..., 0] + GRAY[1] * v[..., 1] + GRAY[2] * v[..., 2] + 8192) >> 14
    return _clamp_rint(v.astype(f32) + np.asarray(a, dtype=f32) * (g[..., None] - v).astype(f32))


def _cell_index(h, w, hl, wl, per_channel):
    """idx [h, w, 3] of the mask / noise draw of every channel value: over [hl][wl](3) cells (hl, wl = h, w: per pixel)"""
    yl = (np.arange(h, dtype=np.int64) * hl) // h
    xl = (np.arange(w, dtype=np.int64) * wl) // w
    cell = yl[:, None] * wl + xl[None, :]
    if per_channel:
        return cell[:, :, None] * 3 + np.arange(3, dtype=np.int64)
    return np.repeat(cell[:, :, None], 3, axis=2)


def op_dropout(v, p, per_channel, seed, hl=None, wl=None):
    h, w = v.shape[:2]
    idx = _cell_index(h, w, hl or h, wl or w, per_channel)
    keep = hash_uniform(seed, idx) >= f32(p)
    return np.where(keep, v, 0)


def op_noise(v, scale, per_channel, seed):
    h, w = v.shape[:2]
    idx = _cell_index(h, w, h, w, per_channel).astype(np.uint64)
    u1, u2 = hash_uniform(seed, 2 * idx), hash_uniform(seed, 2 * idx + 1)
    z = np.sqrt(f32(-2.0) * np.log(f32(1.0) - u1)) * np.cos(f32(2.0 * np.pi) * u2)
    return _clamp_rint(v.astype(f32) + f32(scale) * z.astype(f32))


def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur_axis(img, taps, axis):
    """one pass: (sum q_i v + 32768) >> 16 along ``axis`` with reflect-101 borders"""
    taps = np.asarray(taps, dtype=np.int64)
    r, n = len(taps) // 2, img.shape[axis]
    acc = np.full(img.shape, 32768, dtype=np.int64)
    for i, q in enumerate(taps):
        src = reflect101(np.arange(n) + i - r, n)
        acc += q * np.take(img, src, axis=axis)
    return acc >> 16


def op_blur(v, taps):
    return blur_axis(blur_axis(v, taps, 1), taps, 0)          # horizontal, 8-bit intermediate, then vertical


def apply_plan(images, plan):
    """images uint8 [n, h, w, 3] (numpy), plan: pmoe_amd.augment.AugmentPlan -> uint8 [n, h, w, 3]"""
    out = np.empty_like(images)
    for i in range(images.shape[0]):
        v = images[i].astype(np.int64)
        for s in range(int(plan.n_slots[i])):
            op = int(plan.ops[i, s])
            p = plan.params[i, s].numpy()
            pc, seed = int(plan.per_channel[i, s]), int(plan.seeds[i, s])
            if op == ADD:
                v = op_add(v, p.astype(np.int64))
            elif op == MULTIPLY:
                v = op_multiply(v, p)
            elif op == CONTRAST:
                v = op_contrast(v, p)
            elif op == GRAYSCALE:
                v = op_grayscale(v, p)
            elif op == DROPOUT:
                v = op_dropout(v, p[0], pc, seed)
            elif op == COARSE_DROPOUT:
                v = op_dropout(v, p[0], pc, seed, int(plan.mask_hw[i, s, 0]), int(plan.mask_hw[i, s, 1]))
            elif op == NOISE:
                v = op_noise(v, p[0], pc, seed)
            elif op == BLUR:
                v = op_blur(v, plan.taps[i, :int(plan.blur_k[i])].numpy())
        out[i] = v.astype(np.uint8)
    return out


def to_tensor(images_u8):
    """ToTensor: uint8 [n, h, w, 3] -> float32 [n, 3, h, w] = value / 255"""
    return images_u8.transpose(0, 3, 1, 2).astype(f32) / f32(255.0)
