"""Reference of the U-Net, segmentation-loss and action-head kernels of csrc/punet.hip, csrc/stage1.hip and csrc/stage0.hip, one
function per entry point, with the case tables and input generators of tests/test_unet_kernels_cpu.py and
tests/test_unet_kernels_gpu.py.  The method is that of tests/eca_head_ref.py, whose helpers are used here.

Pure torch on the CPU.  Each function takes what its kernel takes (ld / coff windows, null pointers, the mode) and computes in the
dtype it is handed: float64 is the reference, float32 the plain CPU evaluation that the CPU test holds against the bounds of the
GPU test.  Storage values travel as float64 tensors that hold exactly representable values.  A function returns every buffer its
kernel writes, with NaN where the kernel must not write.  ``mut`` selects a deliberately wrong variant; the CPU test proves that
every one of them is caught.

Bounds of the continuous kind (EPS24 = 2^-24):
  sums      (L + 8) EPS24 sum|term|, L = the longest chain of sequential float32 additions, read from the kernel
  stored    bfloat16: the rounded reference (generators leave nothing near a rounding boundary); float32: 8 EPS24 mag + EPS24 |ref|
  tanhf, expf, logf: T_f units in the last place of the result, carried on by the reference's own derivative

logf of the segmentation criterion takes arguments in (0, 1], a wider range than the [2^-6, e^-2] that T_LOG of eca_head_ref was
measured on.  test_seg_logf_error_is_within_the_constant of tests/test_unet_kernels_gpu.py measures it there: 2^12 frames of one
pixel and two classes, x_t - x_other swept over [-16, 16]; the kernel's own float32 p_t is read back from partT and
-logf(p_t) from partG, and compared with float64 -log of that same float32 p_t.
  measured worst, units in the last place:   logf on (0, 1]  2.039
T_LOG_SEG = twice the measured worst, rounded up to a whole unit.

Left out on purpose: pmoe_history_push and pmoe_mixture_draw (tests/test_policy_tick_gpu.py restates their rules).
"""
import functools

import torch

from tests.eca_head_ref import (BF16, DTYPES, EPS24, F32, F64, T_EXP, T_TANH, ULP, case_id, cdiv, gen,  # noqa: F401
                                grid_stride_entered, hash_uniform, lat, near_boundary, round_to, settle, stored_bound, tname, ve)

MEASURED = {"log_seg": 2.039}               # units in the last place, see the docstring
T_LOG_SEG = 5.0                              # ceil(2 * measured)
NAN = float("nan")
INF = float("inf")
TOL = 2.0 ** -18
GRID_CAPS = {"maxpool2_fwd": 8192, "maxpool2_bwd": 8192, "pixel_shuffle2": 8192, "pixel_unshuffle2": 8192, "copy_window": 8192,
             "add_window": 8192, "cat_windows": 8192, "channel_scale": 8192, "seg_loss_bwd": 16384, "dice_count": 2048}
CAT_ROWS = 32
NCHW_MAX_C = 160 * 1024 // (64 * 4) - 1      # the [64][C + 1] float32 tile in 160 KiB of LDS
EPS_DICE32 = float(torch.tensor(1e-6, dtype=F32))


def nanlike(shape):
    return torch.full(tuple(shape), NAN, dtype=F64)


def esize(dtype):
    return 2 if dtype == BF16 else 4


# ---------------------------------------------------------------------------------------------------------------------------------
# launch routes, from the launch code

def window_route(C, src_ld, src_coff, dst_ld, dst_coff, dtype):
    """copy_window / add_window: whole 16-byte vectors on both sides, or the scalar kernel"""
    v = ve(dtype)
    return "vector" if not (C % v or src_ld % v or src_coff % v or dst_ld % v or dst_coff % v) else "scalar"


def cat_route(src_ld, dst_c, dtype):
    """cat_windows: rows assembled in LDS, or gathered element-wise (torch allocations are 16-byte aligned)"""
    return "lds" if src_ld % ve(dtype) == 0 and CAT_ROWS * dst_c * esize(dtype) <= 48 * 1024 else "element"


def seg_loss_cp(C):
    return -1 if C < 2 or C > 32 else 8 if C <= 8 else 16 if C <= 16 else 24 if C <= 24 else 32


def seg_loss_rows(B, H, W):
    return -1 if min(B, H, W) < 1 else min(B * H, 64) * cdiv(W, 256)


# ---------------------------------------------------------------------------------------------------------------------------------
# MaxPool2d(2, 2) and its backward

def _taps(v, Ho, Wo):
    return [v[:, i:2 * Ho:2, j:2 * Wo:2] for i in (0, 1) for j in (0, 1)]


def _pool_best(v, mut=""):
    """value and tap 0..3 of the maximum in row-major order: the first of equal maxima; a NaN beats everything, the last NaN wins
    (torch's max_pool2d: val > max || isnan(val))"""
    N, H, W, _ = v.shape
    t = _taps(v, H // 2, W // 2)
    m, best = t[0], torch.zeros(t[0].shape, dtype=torch.int64)
    for q in (1, 2, 3):
        if mut == "last":
            take = (t[q] >= m) | torch.isnan(t[q])
        elif mut == "nan":
            take = (t[q] > m) | (torch.isnan(m) & ~torch.isnan(t[q]))
        else:
            take = (t[q] > m) | torch.isnan(t[q])
        m, best = torch.where(take, t[q], m), torch.where(take, torch.tensor(q), best)
    return m, best


def maxpool2s2_fwd(x, C, x_coff=0, mut=""):
    """x [N, H, W, x_ld] -> y [N, H/2, W/2, C] of the window [x_coff, x_coff + C); an odd last row / column is ignored"""
    v = x[..., :C] if mut == "coff" else x[..., x_coff:x_coff + C]
    return {"y": _pool_best(v, mut)[0]}


def maxpool2s2_bwd(x, dy, dskip, C, x_coff, ds_coff, dtype, mut=""):
    """dx [N, H, W, C] = dy at the maximum's tap + the window of dskip (null: nothing), rounded once"""
    v = x[..., x_coff:x_coff + C]
    N, H, W, _ = v.shape
    _, best = _pool_best(v, mut)
    dx = torch.zeros(N, H, W, C, dtype=dy.dtype)
    if dskip is not None and mut != "skip":
        dx += dskip[..., :C] if mut == "coff" else dskip[..., ds_coff:ds_coff + C]
    for q in range(4):
        dx[:, q >> 1::2, q & 1::2] += torch.where(best == q, dy, torch.zeros((), dtype=dy.dtype))
    return {"dx": round_to(dx, dtype)}


# (N, H, W, channel vectors, x as a window, dskip: "null" | "dense" | "window")
POOL_SHAPES = [(2, 2, 2, 1, False, "null"), (2, 6, 10, 3, True, "dense"), (2, 6, 10, 1, False, "window"), (2, 2, 2, 3, True, "window"),
               (2, 5, 7, 3, True, "null"), (2, 5, 7, 1, False, "null")]
POOL_CASES = [c + (d,) for d in DTYPES for c in POOL_SHAPES]


@functools.lru_cache(maxsize=None)
def pool_data(case):
    """multiples of 1/4 up to 2 (sums of two exact in either storage type), channel 1 mod 4 ReLU'd, and planted windows: every
    other window holds, channel by channel (mod 16, shifted from window to window): two equal maxima in each of the six orders, a
    constant, zeros, all -inf, one -inf, one NaN at each of two taps, two NaNs (taps 0 and 2, taps 1 and 3), a NaN with a larger
    value after it"""
    N, H, W, cv, xwin, skip, dtype = case
    C = cv * ve(dtype)
    g = gen("pool", case)
    x = lat(g, (N, H, W, C), 8, 4)
    c = torch.arange(C)
    x[..., c % 4 == 1] = x[..., c % 4 == 1].clamp_min(0)
    plant = [(5, 5, 1, 0), (5, 1, 5, 0), (5, 1, 0, 5), (1, 5, 5, 0), (1, 5, 0, 5), (1, 0, 5, 5), (3, 3, 3, 3), (0, 0, 0, 0),
             (-INF, -INF, -INF, -INF), (1, -INF, 0, 1), (NAN, 1, 2, 0), (1, 2, NAN, 0), (NAN, 1, NAN, 7), (1, NAN, 0, NAN),
             (NAN, 1, 2, 7), (-1, -1, -2, -1)]
    for n in range(N):
        for oy in range(H // 2):
            for ox in range(oy % 2, W // 2, 2):
                for k in range(C):
                    p = plant[(k + 5 * (oy * (W // 2) + ox) + 3 * n) % 16]
                    x[n, 2 * oy, 2 * ox, k], x[n, 2 * oy, 2 * ox + 1, k], x[n, 2 * oy + 1, 2 * ox, k], x[n, 2 * oy + 1, 2 * ox + 1, k] = p
    if xwin:
        x = torch.cat([nanlike((N, H, W, C)), x], -1)
    Ho, Wo = H // 2, W // 2
    dy = lat(g, (N, Ho, Wo, C), 8, 4)
    dy = torch.where(dy == 0, torch.tensor(0.25, dtype=F64), dy)
    ds = {"null": None, "dense": lat(g, (N, H, W, C), 8, 4),
          "window": torch.cat([nanlike((N, H, W, 2 * C)), lat(g, (N, H, W, C), 8, 4)], -1)}[skip]
    return {"x": x, "C": C, "x_coff": C if xwin else 0, "dy": dy, "dskip": ds, "ds_coff": 2 * C if skip == "window" else 0}


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel shuffle / unshuffle, channel windows

def pixel_shuffle2(src, C, dst_ld, dst_coff, mut=""):
    """src [N, H, W, src_ld >= 4C], channel (dy * 2 + dx) * C + k -> dst[n, 2y + dy, 2x + dx, dst_coff + k]"""
    N, H, W, _ = src.shape
    dst = nanlike((N, 2 * H, 2 * W, dst_ld))
    off = 0 if mut == "coff" else dst_coff
    for q in range(4):
        i, j = (q & 1, q >> 1) if mut == "quad" else (q >> 1, q & 1)
        dst[:, i::2, j::2, off:off + C] = src[..., q * C:(q + 1) * C]
    return {"dst": dst}


def pixel_unshuffle2(src, C, src_coff, dst_ld, mut=""):
    """dst[n, y, x, (dy * 2 + dx) * C + k] = src[n, 2y + dy, 2x + dx, src_coff + k], dst [N, H, W, dst_ld >= 4C]"""
    N, H2, W2, _ = src.shape
    dst = nanlike((N, H2 // 2, W2 // 2, dst_ld))
    off = 0 if mut == "coff" else src_coff
    for q in range(4):
        i, j = (q & 1, q >> 1) if mut == "quad" else (q >> 1, q & 1)
        dst[..., q * C:(q + 1) * C] = src[:, i::2, j::2, off:off + C]
    return {"dst": dst}


# (N, H, W, channel vectors, extra source row width in vectors, destination row in multiples of C, destination offset in C)
SHUFFLE_SHAPES = [(2, 1, 1, 1, 0, 1, 0), (2, 3, 5, 2, 1, 3, 1), (2, 3, 5, 1, 2, 3, 0), (2, 1, 1, 2, 0, 3, 1)]
SHUFFLE_CASES = [c + (d,) for d in DTYPES for c in SHUFFLE_SHAPES]


def copy_window(src, src_coff, dst_ld, dst_coff, C, mut=""):
    dst = nanlike((src.shape[0], dst_ld))
    off = 0 if mut == "coff" else src_coff
    dst[:, dst_coff:dst_coff + C] = src[:, off:off + C]
    return {"dst": dst}


def add_window(src, src_coff, dst, dst_coff, C, dtype, mut=""):
    """dst window += src window: one float32 sum, rounded once to the storage type; ``raw`` is the unrounded sum of the window"""
    out = dst.clone()
    off = 0 if mut == "coff" else src_coff
    raw = dst[:, dst_coff:dst_coff + C] + src[:, off:off + C]
    out[:, dst_coff:dst_coff + C] = round_to(raw, dtype)
    return {"dst": out, "raw": raw}


# (rows, C, src_ld, src_coff, dst_ld, dst_coff) in elements, v = the vector of the dtype
def _window_cases():
    out = []
    for d in DTYPES:
        v = ve(d)
        for rows in (1, 7):
            out += [(rows, 2 * v, 4 * v, v, 3 * v, v, d),          # vector form
                    (rows, 23, 32, 8, 40, 8, d),                   # scalar: C = 23
                    (rows, 2 * v, 4 * v, 5, 4 * v, v, d),          # scalar: src_coff = 5
                    (rows, 2 * v, 4 * v, v, 4 * v, 5, d),          # scalar: dst_coff = 5
                    (rows, 2 * v, 28, 0, 4 * v, v, d) if d == BF16 else (rows, 2 * v, 30, 0, 4 * v, v, d)]     # scalar: ld
    return out


WINDOW_CASES = _window_cases()


@functools.lru_cache(maxsize=None)
def window_data(case):
    """randn in the storage type, NaN outside both windows; no bfloat16 sum within TOL of a rounding boundary"""
    rows, C, sld, scoff, dld, dcoff, dtype = case
    g = gen("window", case)
    draw = lambda n: (torch.randn((rows, C), generator=g) * 2).to(dtype).to(F64)       # noqa: E731
    d = {"s": draw("s"), "d": draw("d")}
    d = settle(d, draw, lambda d: {"s": near_boundary(d["s"] + d["d"], TOL * (d["s"].abs() + d["d"].abs()), dtype)})
    src, dst = nanlike((rows, sld)), nanlike((rows, dld))
    src[:, scoff:scoff + C], dst[:, dcoff:dcoff + C] = d["s"], d["d"]
    return {"src": src, "dst": dst}


def cat_windows(srcs, c, src_coff, dst_ld, dst_c, mut=""):
    """dst[r, k c + j] = srcs[k][r, src_coff + j]; zero from K c to dst_c; untouched from dst_c on"""
    K, rows = len(srcs), srcs[0].shape[0]
    dst = nanlike((rows, dst_ld))
    if mut != "pad":
        dst[:, K * c:dst_c] = 0
    off = 0 if mut == "coff" else src_coff
    if mut == "leak":            # every source vector is written out whole, the last window first
        v = 8
        for k in reversed(range(K)):
            a, b = off // v * v, min(cdiv(off + c, v) * v, srcs[k].shape[1])
            lo = k * c - (off - a)
            for j in range(a, b):
                if 0 <= lo + j - a < dst_c:
                    dst[:, lo + j - a] = srcs[k][:, j]
        return {"dst": dst}
    for k in range(K):
        dst[:, k * c:(k + 1) * c] = srcs[k][:, off:off + c]
    return {"dst": dst}


def _cat_cases():
    """(K, c, src_ld, src_coff, dst_c, dst_ld, rows, dtype)"""
    out = []
    for d in DTYPES:
        v = ve(d)
        up = lambda n: cdiv(n, v) * v          # noqa: E731
        for K in (1, 4, 8):
            for c in (23, 32):
                out.append((K, c, 40, 3, up(K * c), up(K * c), 33, d))                  # LDS form, src_coff inside a vector
                out.append((K, c, 40, 8, up(K * c) + 2 * v, up(K * c) + 3 * v, 31, d))    # wider dst_c and dst_ld > dst_c
        out += [(4, 23, 40, 3, up(92), up(92), 1, d), (4, 23, 40, 3, up(92), up(92), 32, d),
                (4, 23, 37, 3, up(92), up(92) + v, 33, d),                               # pitch no multiple of the vector: element-wise
                (2, 32, 40, 5, 48 * 1024 // (32 * esize(d)) + v, 48 * 1024 // (32 * esize(d)) + v, 33, d)]   # just over 48 KiB
    return out


CAT_CASES = _cat_cases()


@functools.lru_cache(maxsize=None)
def cat_data(case):
    K, c, sld, scoff, dst_c, dst_ld, rows, dtype = case
    g = gen("cat", case)
    srcs = []
    for _ in range(K):
        s = nanlike((rows, sld))
        s[:, scoff:scoff + c] = lat(g, (rows, c), 64, 4)
        srcs.append(s)
    return {"srcs": tuple(srcs)}


def nhwc_to_nchw(src, C, src_coff, mut=""):
    """src [N, H, W, ld] window -> float32 [N, C, H, W]"""
    off = 0 if mut == "coff" else src_coff
    return {"dst": src[..., off:off + C].permute(0, 3, 1, 2).contiguous()}


# (N, HW, C, ld, coff)
NCHW_SHAPES = [(2, hw, c, c + 9, 4) for hw in (1, 63, 64, 65, 130) for c in (1, 23, 138)] + \
              [(1, 65, NCHW_MAX_C, NCHW_MAX_C, 0), (2, 130, 23, 23, 0)]
NCHW_CASES = [c + (d,) for d in DTYPES for c in NCHW_SHAPES]


@functools.lru_cache(maxsize=None)
def nchw_data(case):
    N, HW, C, ld, coff, dtype = case
    src = nanlike((N, 1, HW, ld))
    src[..., coff:coff + C] = lat(gen("nchw", case), (N, 1, HW, C), 64, 4)
    return {"src": src}


# ---------------------------------------------------------------------------------------------------------------------------------
# Dropout2d and the dice score (stage0.hip)

def dropout2d_table(N, C, p, seed, mut=""):
    """table[n, c] = hash_uniform(seed, n C + c) >= p ? 1.f / (1.f - p) : 0, all in float32; p = 1 keeps nothing"""
    pf = torch.tensor(p, dtype=F32)
    u = hash_uniform(seed, N * C).reshape(N, C)
    if mut == "ctr":
        u = hash_uniform(seed, C)[None].expand(N, C)
    keep = (u > pf.to(F64)) if mut == "gt" else (u >= pf.to(F64))
    scale = (1 / (1 - pf)).to(F64) if p < 1 else torch.zeros((), dtype=F64)
    if mut == "noscale":
        scale = torch.ones((), dtype=F64)
    return {"table": torch.where(keep, scale, torch.zeros((), dtype=F64))}


DROPOUT_CASES = [(n, c, p, s) for n, c in ((1, 1), (2, 128), (1, 257), (8, 125)) for p in (0.0, 0.3, 0.5, 1.0)
                 for s in (5, (1 << 40) + 12345)]


def channel_scale(x, table, C, coff, dtype, mut=""):
    """x[n, p, coff + k] *= table[n, k] in place; ``raw`` is the unrounded product of the window"""
    out = x.clone()
    off = 0 if mut == "coff" else coff
    raw = x[..., off:off + C] * table[:, None, :]
    out[..., off:off + C] = round_to(raw, dtype)
    return {"x": out, "raw": raw}


SCALE_CASES = [(2, hw, cv * ve(d), win, d) for d in DTYPES for hw in (1, 7) for cv in (1, 3) for win in (False, True)]
TABLE_VALUES = (0.0, 2.0, float(torch.tensor(1.0, dtype=F32) / torch.tensor(0.7, dtype=F32)))


@functools.lru_cache(maxsize=None)
def scale_data(case):
    N, HW, C, win, dtype = case
    g = gen("scale", case)
    table = torch.tensor(TABLE_VALUES, dtype=F64)[torch.randint(0, 3, (N, C), generator=g)]
    table[0, :3] = torch.tensor(TABLE_VALUES, dtype=F64)[:min(C, 3)]
    draw = lambda n: torch.randn((N, HW, C), generator=g).to(dtype).to(F64)       # noqa: E731
    d = settle({"v": draw("v")}, draw, lambda d: {"v": near_boundary(d["v"] * table[:, None], TOL * (d["v"] * table[:, None]).abs(), dtype)})
    x = d["v"]
    if win:
        x = torch.cat([nanlike((N, HW, C)), x, nanlike((N, HW, ve(dtype)))], -1)
    return {"x": x, "table": table, "coff": C if win else 0}


def dice_score(logits, target, eps, mut=""):
    """logits [B, C, HW], target [B, HW] -> counts int64 [3, C] (arg-max & target, arg-max, target; lowest index on ties; a target
    outside [0, C) counts nowhere) and dice = 2 (inter + eps) / (pred + target + eps) in the dtype of the logits"""
    B, C, HW = logits.shape
    am = logits.argmax(1) if mut != "last" else C - 1 - logits.flip(1).argmax(1)
    cls = torch.arange(C)[:, None, None]
    p, t = am[None] == cls, target[None] == cls
    counts = torch.stack([(p & t).sum((1, 2)), p.sum((1, 2)), t.sum((1, 2))])
    e = torch.tensor(eps, dtype=F32).to(logits.dtype)
    cf = counts.to(logits.dtype)
    uni = (cf[1] + cf[2]) + (0 if mut == "noeps" else e)
    return {"counts": counts, "dice": 2 * (cf[0] + e) / uni}


DICE_CASES = [(2, c, hw, e) for c in (1, 2, 23, 64) for hw in (1, 255, 257) for e in (1e-6, 0.5)]
DICE_BIG = (1, 2, 2048 * 256 + 77, 1e-6)


@functools.lru_cache(maxsize=None)
def dice_data(case):
    """logits on multiples of 1/2 in [-2, 2] (ties everywhere), class C - 1 never the arg-max nor a target where C >= 3 (absent from
    both), a tenth of the targets outside [0, C)"""
    B, C, HW, eps = case
    g = gen("dice", case)
    x = lat(g, (B, C, HW), 4, 2)
    t = torch.randint(0, C, (B, HW), generator=g)
    if C >= 3:
        x[:, C - 1] = -3.0
        t = t.clamp_max(C - 2)
    out = torch.rand(B, HW, generator=g) < 0.1
    t = torch.where(out, torch.where(torch.rand(B, HW, generator=g) < 0.5, torch.tensor(-1), torch.tensor(C)), t)
    return {"logits": x, "target": t}


# ---------------------------------------------------------------------------------------------------------------------------------
# tanh action head, action loss, PMoE blend (punet.hip)

B_CASES = (1, 255, 256, 257, 600)
HEAD_CASES = [(B, hld, sld, d) for d in DTYPES for B in B_CASES for hld, sld in ((2, 1), (16, 4))]
KINDS = ("lattice", "continuous")
LOSS_C = (0.75, 0.25)


def chain256(n):
    """sequential additions of one thread of a loop i += 256 over n items"""
    return cdiv(n, 256)


def action_head_fwd(head, spd, B):
    """actions[b] = tanh(head[b, 0:2]), speeds[b] = spd[b, 0]"""
    return {"actions": torch.tanh(head[:B, :2]), "speeds": spd[:B, 0].clone()}


def action_head_fwd_bounds(ref):
    return {"actions": T_TANH * ULP * ref["actions"].abs()}


def action_head_bwd(actions, dact, dspeeds, rows, head_ld, spd_ld, B, dtype, mut=""):
    """whole rows: dhead[b, 0:2] = dact (1 - a^2), zeros beyond; dspd[b, 0] = dspeeds, zeros beyond; rows from B on untouched"""
    dh, ds = nanlike((rows, head_ld)), nanlike((rows, spd_ld))
    dh[:B], ds[:B] = 0, 0
    raw = torch.zeros(B, 2, dtype=actions.dtype)
    if dact is not None:
        raw = dact * (1 - actions * actions)
        dh[:B, :2] = round_to(raw, dtype).to(F64)
    if dspeeds is not None:
        ds[:B, 0] = round_to(dspeeds, dtype).to(F64)
    mag = (dact.abs() * (1 + actions * actions)) if dact is not None else raw
    return {"dhead": dh, "dspd": ds, "raw": raw, "mag": mag}


@functools.lru_cache(maxsize=None)
def head_data(case, kind):
    """lattice: head in {0, +-16, +-24} (tanhf exact), gradients multiples of 1/4.  continuous: |z| <= 9; the gradients are
    redrawn until no bfloat16 result is within TOL of a rounding boundary.  Rows beyond B hold NaN.  ``actions`` is the input of the
    backward pass: the forward reference rounded to float32."""
    B, hld, sld, dtype = case
    g = gen("head", case, kind)
    rows = B + 3
    head, spd = nanlike((rows, hld)), nanlike((rows, sld))
    if kind == "lattice":
        head[:B] = torch.tensor([0.0, 16.0, -16.0, 24.0, -24.0], dtype=F64)[torch.randint(0, 5, (B, hld), generator=g)]
        spd[:B] = lat(g, (B, sld), 8, 4)
        draw = lambda n: lat(g, (B, 2) if n == "dact" else (B,), 8, 4)       # noqa: E731
    else:
        head[:B] = (torch.rand((B, hld), generator=g, dtype=F64) * 18 - 9).to(dtype).to(F64)
        spd[:B] = (torch.randn((B, sld), generator=g) * 3).to(dtype).to(F64)
        draw = lambda n: torch.randn((B, 2) if n == "dact" else (B,), generator=g).to(F32).to(F64)       # noqa: E731
    actions = round_to(torch.tanh(head[:B, :2]), F32)
    if dtype == BF16:        # 1 - a^2 below 2^-6 cancels in float32 and no bfloat16 rounding of it is certain: such actions become +-1
        actions = torch.where(1 - actions * actions < 2.0 ** -6, torch.sign(actions), actions)
    d = {"dact": draw("dact"), "dspeeds": draw("dspeeds")}

    def amb(d):
        r = action_head_bwd(actions, d["dact"], d["dspeeds"], rows, hld, sld, B, F64)
        return {"dact": near_boundary(r["raw"], TOL * r["mag"], dtype), "dspeeds": near_boundary(d["dspeeds"], TOL * d["dspeeds"].abs(), dtype)}
    d = settle(d, draw, amb)
    return {"head": head, "spd": spd, "actions": actions, "rows": rows, **d}


def action_loss(actions, speeds, act_gt, spd_gt, c0, c1, B, mut=""):
    """c0 mean|a - a_gt| (+ c1 mean (s - s_gt)^2) with its gradients; speeds None: the L1 term alone, dspeeds untouched"""
    d = actions - act_gt
    sign = torch.sign(d)
    if mut == "l1sign":
        sign = torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))
    nb = B if mut == "halfB" else 2 * B
    out = {"loss": c0 * d.abs().sum() / nb, "dact": c0 * sign / nb, "l1": d.abs().sum(), "l2": torch.zeros((), dtype=d.dtype),
           "dspeeds": None}
    if speeds is not None:
        e = speeds - spd_gt
        out["l2"] = (e * e).sum()
        out["loss"] = out["loss"] + c1 * out["l2"] / B
        out["dspeeds"] = c1 * 2 * e / B
    return out


def action_loss_bounds(ref, c0, c1, B, kind):
    """l1: ceil(2B / 256) sequential additions per thread, l2: ceil(B / 256), then the 8 levels of the tree; one rounding per
    |d| (one more unit of the factor), three per d^2; then a product, a division and a sum per term of the loss (8 EPS24 covers them
    and a division that is not correctly rounded).  On the lattice the sums are exact and only the last line remains."""
    s = 0.0 if kind == "lattice" else 1.0
    b1 = s * (chain256(2 * B) + 8 + 1) * EPS24 * ref["l1"]
    b2 = s * (chain256(B) + 8 + 3) * EPS24 * ref["l2"]
    t1, t2 = c0 * ref["l1"] / (2 * B), c1 * ref["l2"] / B
    out = {"loss": c0 * b1 / (2 * B) + c1 * b2 / B + 8 * EPS24 * (t1 + t2), "dact": 4 * EPS24 * ref["dact"].abs()}
    if ref["dspeeds"] is not None:
        out["dspeeds"] = 8 * EPS24 * ref["dspeeds"].abs()
    return out


LOSS_CASES = [(B, s) for B in B_CASES for s in (False, True)]


@functools.lru_cache(maxsize=None)
def loss_data(case, kind):
    """lattice: actions in {0, +-1}, everything else multiples of 1/4 (every sum exact).  Every fifth action equals its target."""
    B, with_speed = case
    g = gen("action_loss", case, kind)
    if kind == "lattice":
        a = torch.randint(-1, 2, (B, 2), generator=g).to(F64)
        gt, s, sg = lat(g, (B, 2), 4, 4), lat(g, (B,), 8, 4), lat(g, (B,), 8, 4)
    else:
        a = torch.tanh(torch.randn((B, 2), generator=g)).to(F32).to(F64)
        gt = (torch.rand((B, 2), generator=g) * 2 - 1).to(F32).to(F64)
        s, sg = (torch.randn((B,), generator=g) * 3).to(F32).to(F64), (torch.randn((B,), generator=g) * 3).to(F32).to(F64)
    eq = (torch.arange(2 * B).reshape(B, 2) % 5) == 0
    gt = torch.where(eq, a, gt)
    return {"actions": a, "gt": gt, "speeds": s if with_speed else None, "spd_gt": sg if with_speed else None}


def blend_fwd(moe, pu, lat_w, lat_b, long_w, long_b, mut=""):
    """out[b, j] = tanh(w_j[0] moe[b, j] + w_j[1] pu[b, j] + bias_j), j = 0 lateral, 1 longitudinal"""
    w = torch.stack([lat_w, long_w])
    bias = torch.stack([lat_b[0], long_b[0]])
    z = w[:, 0] * moe + w[:, 1] * pu + bias
    return {"out": torch.tanh(z), "zmag": (w[:, 0] * moe).abs() + (w[:, 1] * pu).abs() + bias.abs()}


def blend_fwd_bounds(ref):
    """z: two products and two sums in float32 (4 EPS24 zmag); tanhf T_TANH units; z's error through 1 - out^2 (+ second order)"""
    dz = 4 * EPS24 * ref["zmag"]
    o = ref["out"]
    return {"out": T_TANH * ULP * o.abs() + (1 - o * o + 2 * dz) * dz}


def blend_bwd(moe, pu, lat_w, long_w, out, dout, with_dpu=True, mut=""):
    """g = dout (1 - out^2); dW_j = sum_b g [moe, pu], db_j = sum_b g, dpunet = g w_j[1]"""
    g = dout * (1 - out * out)
    w = torch.stack([lat_w, long_w])
    terms = torch.stack([g * moe, g * pu, g], -1)                  # [B, 2, 3]
    r = {"sums": terms.sum(0), "sums_abs": terms.abs().sum(0), "gmag": dout.abs() * (1 + out * out), "g": g,
         "dpu": (g * w[:, 0 if mut == "w0" else 1]) if with_dpu else None}
    r["term_mag"] = torch.stack([r["gmag"] * moe.abs(), r["gmag"] * pu.abs(), r["gmag"]], -1).sum(0)
    return r


def blend_bwd_bounds(ref, long_w, lat_w, B, kind):
    """g: three float32 roundings (4 EPS24 gmag); a term one more; the sum ceil(B / 256) + 8 levels"""
    if kind == "lattice":
        z = torch.zeros_like(ref["sums"])
        return {"sums": z, "dpu": torch.zeros_like(ref["g"])}
    w1 = torch.stack([lat_w, long_w])[:, 1].abs()
    return {"sums": (chain256(B) + 8) * EPS24 * ref["sums_abs"] + 5 * EPS24 * ref["term_mag"],
            "dpu": 4 * EPS24 * ref["gmag"] * w1 + EPS24 * (ref["g"] * w1).abs()}


BLEND_CASES = list(B_CASES)


@functools.lru_cache(maxsize=None)
def blend_data(B, kind):
    """lattice: integer actions, weights and biases multiples of 16: z is 0 or |z| >= 16, where tanhf is 0 or +-1 exactly"""
    g = gen("blend", B, kind)
    if kind == "lattice":
        moe, pu = torch.randint(-2, 3, (B, 2), generator=g).to(F64), torch.randint(-2, 3, (B, 2), generator=g).to(F64)
        w = {"lat_w": torch.tensor([16.0, 32.0]), "lat_b": torch.tensor([0.0]), "long_w": torch.tensor([-16.0, 16.0]),
             "long_b": torch.tensor([16.0])}
        dout = lat(g, (B, 2), 8, 4)
        moe[0], pu[0] = torch.tensor([0.0, 1.0], dtype=F64), 0.0          # z = 0 in both columns of row 0
    else:
        moe, pu = (torch.randn((B, 2), generator=g)).to(F32).to(F64), torch.tanh(torch.randn((B, 2), generator=g)).to(F32).to(F64)
        w = {"lat_w": torch.tensor([0.75, -1.25]), "lat_b": torch.tensor([0.125]), "long_w": torch.tensor([-0.5, 1.5]),
             "long_b": torch.tensor([-0.25])}
        dout = torch.randn((B, 2), generator=g).to(F32).to(F64)
    w = {k: v.to(F64) for k, v in w.items()}
    out = round_to(blend_fwd(moe, pu, **w)["out"], F32)
    return {"moe": moe, "pu": pu, "dout": dout, "out": out, **w}


# ---------------------------------------------------------------------------------------------------------------------------------
# AutoregressiveCriterion (stage1.hip)

SEG_MODES = ("tversky", "l1", "l2")
SEG_SHAPES = [(1, 1, 2, 1, 1), (2, 2, 8, 3, 5), (1, 1, 9, 4, 7), (2, 1, 16, 5, 256), (1, 2, 17, 7, 257), (2, 1, 24, 33, 9),
              (1, 1, 25, 2, 3), (1, 3, 32, 3, 300)]
SEG_BIG = (1, 1, 2, 2049, 2048)
SEG_DEFAULTS = (0.5, 0.5, 0.5, 0.5)           # ce_weight, tversky_weight, alpha, beta
SEG_OTHER = (0.25, 0.75, 0.25, 0.75)          # exact in float32


def seg_geometry(B, H, W, C):
    """rows one thread walks, row splits, column blocks, partial rows"""
    rows = B * H
    nsplit = min(rows, 64)
    xb = cdiv(W, 256)
    walk = max((rows * (s + 1)) // nsplit - (rows * s) // nsplit for s in range(nsplit))
    return {"walk": walk, "nsplit": nsplit, "xb": xb, "NS": nsplit * xb}


def seg_loss_fwd(logits, target, mode, ce_w=0.5, tv_w=0.5, alpha=0.5, beta=0.5, mut="", w_f32=False):
    """logits [B, F, C, H, W], target [B, F, H, W].  Returns loss [1 + F], and in the tversky mode coefG [F, 32], coefT [F, 2, CP, W]
    (NaN for the padded classes, which finalize does not write), partG [F, 4, 32] and partT [F, 3, CP, W] summed over their partition
    axis, with the intermediate quantities the bounds need.  ``w_f32``: the class-dice weights in float32, as the oracle forms
    them."""
    B, F, C, H, W = logits.shape
    dt = logits.dtype
    CP = seg_loss_cp(C)
    cls = torch.arange(C)
    onehot = (target[:, :, None] == cls[None, None, :, None, None])            # [B, F, C, H, W]
    oh = onehot.to(dt)
    partG = torch.zeros(F, 4, 32, dtype=dt)
    if mode != "tversky":
        d = logits - oh
        term = d.abs() if mode == "l1" else d * d
        partG[:, 0, 0] = term.sum((0, 2, 3, 4))
        per = partG[:, 0, 0] / (B * C * H * W)
        return {"loss": torch.cat([per.sum()[None], per]), "partG": partG, "term": term}
    x = logits
    if mut == "padded":        # the padded lanes take part in the soft-max as logits of 0
        x = torch.cat([logits, torch.zeros(B, F, CP - C, H, W, dtype=dt)], 2)
    p = torch.softmax(x, 2)[:, :, :C]
    am = logits.argmax(2)                                                       # lowest index on ties
    amh = (am[:, :, None] == cls[None, None, :, None, None])
    nl = -torch.log((p * oh).sum(2))                                            # [B, F, H, W]
    partG[:, 0, :C] = amh.sum((0, 3, 4)).to(dt)
    partG[:, 1, :C] = (amh & onehot).sum((0, 3, 4)).to(dt)
    partG[:, 2, :C] = (nl[:, :, None] * oh).sum((0, 3, 4))
    partG[:, 3, :C] = onehot.sum((0, 3, 4)).to(dt)
    partT = torch.zeros(F, 3, CP, W, dtype=dt)
    red = (0, 3, 4) if mut == "cols" else (0, 3)
    keep = mut == "cols"
    n, I, P = (t.sum(red, keepdim=keep) for t in (oh, p * oh, p))
    if keep:
        n, I, P = (t[0, :, :, 0].expand(F, C, W) for t in (n, I, P))
    partT[:, 0, :C], partT[:, 1, :C], partT[:, 2, :C] = n, I, P
    D = I + alpha * (P - I) + beta * (n - I)
    k = tv_w / (C * W)
    coefT = torch.full((F, 2, CP, W), NAN, dtype=dt)
    a0, a1 = -k * (alpha * P + beta * n) / (D * D), k * alpha * I / (D * D)
    coefT[:, 0, :C], coefT[:, 1, :C] = (a1, a0) if mut == "coefswap" else (a0, a1)
    g = partG
    if w_f32:
        e32 = torch.tensor(1e-6, dtype=F32)
        wc = (1 - 2 * (g[:, 1, :C].to(F32) + e32) / (g[:, 0, :C].to(F32) + g[:, 3, :C].to(F32) + e32)).to(dt)
    else:
        e = EPS_DICE32
        wc = 1 - 2 * ((0 if mut == "nointer" else g[:, 1, :C]) + e) / (g[:, 0, :C] + g[:, 3, :C] + e)
    num, den = (wc * g[:, 2, :C]).sum(1), (wc * g[:, 3, :C]).sum(1)
    if mut == "cenorm":
        den = torch.full_like(den, B * H * W)
    coefG = torch.zeros(F, 32, dtype=dt)
    coefG[:, :C] = ce_w * wc / den[:, None]
    ratio = I / D
    per = ce_w * num / den + tv_w * (1 - ratio.sum((1, 2)) / (C * W))
    return {"loss": torch.cat([per.sum()[None], per]), "coefG": coefG, "coefT": coefT, "partG": partG, "partT": partT,
            "p": p, "nl": nl, "target": target, "wc": wc, "num": num, "den": den, "D": D, "ratio": ratio, "am": am}


def seg_loss_bwd(logits, target, coefG, coefT, dloss, mode, mut=""):
    """dlogits from the coefficients of the forward pass (the analytic form the kernel uses)"""
    B, F, C, H, W = logits.shape
    dt = logits.dtype
    up = 1.0 if dloss is None else dloss
    oh = (target[:, :, None] == torch.arange(C)[None, None, :, None, None]).to(dt)
    if mode != "tversky":
        d = logits - oh
        sign = torch.sign(d)
        if mut == "l1sign":
            sign = torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))
        return {"dlogits": up * (sign if mode == "l1" else 2 * d) / (B * C * H * W)}
    p = torch.softmax(logits, 2)
    c0, c1 = coefT[None, :, 0, :C, None, :], coefT[None, :, 1, :C, None, :]          # [1, F, C, 1, W]
    dp = c1 + oh * c0
    dot = (p * dp).sum(2, keepdim=True)
    kce = (coefG[None, :, :C, None, None] * oh).sum(2, keepdim=True)
    t1, t2 = kce * (p - oh), p * (dp - dot)
    return {"dlogits": up * (t1 + t2), "p": p, "dp": dp, "dot": dot, "kce": kce, "oh": oh,
            "dpmag": c1.abs() + oh * c0.abs(), "dotmag": (p * dp.abs()).sum(2, keepdim=True)}


def seg_rp(C, kind):
    """relative error of a soft-max probability: expf T_EXP units on numerator and sum, the sum's C - 1 additions, the reciprocal
    (2 EPS24, not relied on to be correctly rounded) and the product; x - max is exact for the generators' logits.  Lattice: 0."""
    return 0.0 if kind == "lattice" else 2 * T_EXP * ULP + (C + 2) * EPS24


def seg_loss_bounds(ref, shape, mode, kind, ce_w=0.5, tv_w=0.5, alpha=0.5, beta=0.5):
    """bounds of what seg_loss_fwd returns, step by step as the kernels compute them"""
    B, F, C, H, W = shape
    geo = seg_geometry(B, H, W, C)
    E = EPS24
    if mode != "tversky":
        # one thread adds C terms per row of its walk; 6 shuffle steps, 3 additions over the waves, NS rows in finalize;
        # a term: one rounding of x - onehot, for l2 two more of the square
        L = geo["walk"] * C + 6 + 3 + geo["NS"]
        s = 0.0 if kind == "lattice" else 1.0
        S = ref["partG"][:, 0, 0]
        bS = s * (L + 8 + 3) * E * S
        per = ref["loss"][1:]
        bper = bS / (B * C * H * W) + 6 * E * per.abs()
        bG = torch.zeros_like(ref["partG"])
        bG[:, 0, 0] = bS
        return {"partG": bG, "loss": torch.cat([(bper.sum() + F * E * per.abs().sum())[None], bper])}
    rp = seg_rp(C, kind)
    g, pt = ref["partG"], ref["partT"]
    n, I, P = pt[:, 0, :C], pt[:, 1, :C], pt[:, 2, :C]
    LT = geo["walk"]                                   # the row walk of one thread; the partition axis is summed in float64
    fs = 0.0 if kind == "lattice" else 1.0
    bI, bP = fs * ((LT + 8) * E + rp) * I, fs * ((LT + 8) * E + rp) * P
    bT = torch.zeros_like(pt)
    bT[:, 1, :C], bT[:, 2, :C] = bI, bP
    # finalize sums the nsplit partial rows again in float32
    bI2, bP2 = bI + fs * geo["nsplit"] * E * I, bP + fs * geo["nsplit"] * E * P
    D = ref["D"]
    Dmag = I + alpha * (P + I) + beta * (n + I)
    bD = abs(1 - alpha - beta) * bI2 + alpha * bP2 + 6 * E * Dmag
    ratio = ref["ratio"]
    bratio = bI2 / D + I * bD / (D * D) + 2 * E * ratio
    Lr = cdiv(C * W, 256)
    brsum = (Lr + 8) * E * ratio.sum((1, 2)) + bratio.sum((1, 2))
    k = tv_w / (C * W)
    cT = ref["coefT"][:, :, :C]
    bcT = torch.zeros_like(ref["coefT"])
    bcT[:, 0, :C] = k * (alpha * bP2 / D ** 2 + 2 * (alpha * P + beta * n) * bD / D ** 3) + 8 * E * cT[:, 0].abs()
    bcT[:, 1, :C] = k * alpha * (bI2 / D ** 2 + 2 * I * bD / D ** 3) + 8 * E * cT[:, 1].abs()
    # class sums of -log p_t: logf T_LOG_SEG units, and the error of p_t through 1 / p_t; the chain: walk, 6 shuffles, 3 waves, NS rows
    LG = geo["walk"] + 6 + 3 + geo["NS"]
    ga = g[:, 2, :C]
    nlerr = T_LOG_SEG * ULP * ref["nl"].abs() + rp * 1.0000001
    oh = (ref["target"][:, :, None] == torch.arange(C)[None, None, :, None, None]).to(F64)
    bga = (LG + 8) * E * ga + (nlerr[:, :, None] * oh).sum((0, 3, 4))
    bG = torch.zeros_like(g)
    bG[:, 2, :C] = bga
    wc = ref["wc"]
    q = 1 - wc                                          # 2 (inter + eps) / (pred + target + eps)
    bw = 5 * E * (q.abs() + wc.abs())
    num, den = ref["num"], ref["den"]
    bnum = (bw * ga + wc.abs() * bga).sum(1) + (C + 2) * E * (wc.abs() * ga).sum(1)
    bden = (bw * g[:, 3, :C]).sum(1) + (C + 2) * E * (wc.abs() * g[:, 3, :C]).sum(1)
    bcG = torch.zeros_like(ref["coefG"])
    bcG[:, :C] = ce_w * (bw / den.abs()[:, None] + wc.abs() * bden[:, None] / (den ** 2)[:, None]) + 4 * E * ref["coefG"][:, :C].abs()
    tv = 1 - ratio.sum((1, 2)) / (C * W)
    bper = ce_w * (bnum / den.abs() + num.abs() * bden / den ** 2) + tv_w * brsum / (C * W) + \
        6 * E * ((ce_w * num / den).abs() + tv_w * (1 + ratio.sum((1, 2)) / (C * W)))
    per = ref["loss"][1:]
    return {"partG": bG, "partT": bT, "coefG": bcG, "coefT": bcT,
            "loss": torch.cat([(bper.sum() + F * E * per.abs().sum())[None], bper]), "tv": tv}


def seg_loss_bwd_bounds(ref, shape, mode, kind, dloss):
    """per pixel, from coefficients that are the launch's inputs: p with seg_rp, dp one addition, dot C products and additions"""
    B, F, C, H, W = shape
    E = EPS24
    up = 1.0 if dloss is None else abs(dloss)
    if mode != "tversky":
        return {"dlogits": 8 * E * ref["dlogits"].abs()}
    rp = seg_rp(C, kind)
    p, dp, dot, kce, oh = ref["p"], ref["dp"], ref["dot"], ref["kce"], ref["oh"]
    bdp = E * ref["dpmag"]
    bdot = (rp + (C + 2) * E) * ref["dotmag"] + (p * bdp).sum(2, keepdim=True)
    b = kce.abs() * (rp * p + E * (p - oh).abs()) + rp * p * (dp - dot).abs() + p * (bdp + bdot) + \
        4 * E * ((kce * (p - oh)).abs() + p * (dp.abs() + dot.abs()))
    # (lattice: a class 256 below the top has p = e^-256 in float64 and 0 in float32)
    return {"dlogits": up * b + E * ref["dlogits"].abs() + (1e-100 if kind == "lattice" else 0.0)}


def seg_conditions(ref, shape, alpha=0.5, beta=0.5):
    """the three conditions of the continuous kind, on the final inputs"""
    B, F, C, H, W = shape
    g, pt = ref["partG"], ref["partT"]
    dice = 1 - ref["wc"]
    present = (g[:, 0, :C] + g[:, 3, :C]) > 0
    n, I, P = pt[:, 0, :C], pt[:, 1, :C], pt[:, 2, :C]
    big = torch.maximum(I, torch.maximum(alpha * P, beta * n))
    wn = ref["wc"] * g[:, 3, :C]
    return {"dice": bool((dice[present] <= 0.9).all()),
            "den": bool((wn.sum(1).abs() >= 0.1 * wn.abs().sum(1)).all() and (wn.abs().sum(1) > 0).all()),
            "tversky": bool((ref["D"] >= 2.0 ** -10 * big).all() and (ref["D"] > 0).all())}


@functools.lru_cache(maxsize=None)
def seg_data(shape, kind, mode="tversky"):
    """logits [B, F, C, H, W], target [B, F, H, W].
    lattice: per pixel a power-of-two number of classes share the top logit (a multiple of 1/4), the rest lie 256 below; the
    target is one of the top classes.  In the l1 / l2 modes the logits are multiples of 1/4 in [-2, 2], exact 0 and 1 included.
    continuous: multiples of 2^-12 in [-8, 8] (x - max is exact in float32 and lies in [-16, 0]); the target is the arg-max at
    about 4 pixels of 10 and another class elsewhere, redrawn as a whole until seg_conditions holds."""
    B, F, C, H, W = shape
    for attempt in range(64):
        g = gen("seg", shape, kind, mode, attempt)
        if kind == "lattice" and mode != "tversky":
            x = lat(g, (B, F, C, H, W), 8, 4)
            t = torch.randint(0, C, (B, F, H, W), generator=g)
            return {"logits": x, "target": t}
        if kind == "lattice":
            # row r of a column holds a circular window of G (or 2G) top classes that starts at r G + shift: the windows of one
            # column cover every class, so no Tversky denominator is 0
            R_, G = B * H, 1
            while G * R_ < C:
                G *= 2
            r = (torch.arange(B)[:, None] * H + torch.arange(H)[None]).reshape(B, 1, H, 1)
            shift = torch.randint(0, C, (1, F, 1, W), generator=g)
            dbl = torch.randint(0, 2, (B, F, H, W), generator=g) if 2 * G <= C else torch.zeros(B, F, H, W, dtype=torch.int64)
            size, start = G * (1 + dbl), (r * G + shift) % C
            cidx = torch.arange(C)[None, None, :, None, None]
            top = ((cidx - start[:, :, None]) % C) < size[:, :, None]
            base = lat(g, (B, F, 1, H, W), 8, 4)
            x = torch.where(top, base, base - 256)
            t = (start + (torch.rand((B, F, H, W), generator=g, dtype=F64) * size).long().clamp_max(2 * G - 1) % size) % C
            t = torch.where(torch.rand((B, F, H, W), generator=g) < 0.5, x.argmax(2), t)      # the arg-max: the lowest top class
            return {"logits": x, "target": t}
        x = torch.randint(-8 * 4096, 8 * 4096 + 1, (B, F, C, H, W), generator=g).to(F64) / 4096
        am = x.argmax(2)
        other = (am + torch.randint(1, C, (B, F, H, W), generator=g)) % C
        t = torch.where(torch.rand((B, F, H, W), generator=g) < 0.4, am, other)
        if B * F * H * W == 1:
            t = other
        d = {"logits": x, "target": t}
        if mode != "tversky":
            return d
        if all(seg_conditions(seg_loss_fwd(x, t, "tversky"), shape).values()):
            return d
    raise AssertionError("no inputs that meet the conditions")


SEG_LOGF_F = 1 << 12


def seg_logf_data():
    """2^12 frames of one pixel and two classes: x_t - x_other sweeps [-16, 16], so p_t sweeps (0, 1)"""
    d = (torch.rand(SEG_LOGF_F, generator=gen("seg_logf"), dtype=F64) * 32 - 16).to(F32).to(F64)
    x = torch.zeros(1, SEG_LOGF_F, 2, 1, 1, dtype=F64)
    t = torch.randint(0, 2, (1, SEG_LOGF_F, 1, 1), generator=gen("seg_logf_t"))
    x[0, :, :, 0, 0] = torch.where(torch.arange(2)[None] == t[0, :, 0], d[:, None], torch.zeros((), dtype=F64))
    return {"logits": x, "target": t}


# ---------------------------------------------------------------------------------------------------------------------------------
# grid-stride cases: just above cap x 256 items with a ragged tail, float32 (a 16-byte vector is an item whatever the type)

BIG_ITEMS = 8192 * 256 + 3
# kernel -> (items of the launch, shape parameters)
BIG_CASES = {
    "maxpool2_fwd": (BIG_ITEMS, dict(N=1, H=2, W=2 * BIG_ITEMS, C=4)),
    "maxpool2_bwd": (BIG_ITEMS, dict(N=1, H=2, W=2 * BIG_ITEMS, C=4)),       # x, dx: 4 vectors per item, dy one: 302 MB
    "pixel_shuffle2": (4 * (BIG_ITEMS // 4 + 1), dict(N=1, H=1, W=BIG_ITEMS // 4 + 1, C=4)),
    "pixel_unshuffle2": (4 * (BIG_ITEMS // 4 + 1), dict(N=1, H=1, W=BIG_ITEMS // 4 + 1, C=4)),
    "copy_window/vector": (BIG_ITEMS, dict(rows=BIG_ITEMS, C=4, ld=4)),
    "copy_window/scalar": (BIG_ITEMS, dict(rows=BIG_ITEMS, C=1, ld=1)),
    "add_window/vector": (BIG_ITEMS, dict(rows=BIG_ITEMS, C=4, ld=4)),
    "add_window/scalar": (BIG_ITEMS, dict(rows=BIG_ITEMS, C=1, ld=1)),
    "cat_windows": (BIG_ITEMS, dict(rows=BIG_ITEMS, K=1, c=3, src_ld=5, dst_c=4)),
    "channel_scale": (BIG_ITEMS, dict(N=1, HW=BIG_ITEMS, C=4)),
}


def dropout_hit_case():
    """p equal to one of the table's own uniforms (a float32 multiple of 2^-24): the only place where >= and > differ"""
    seed = 5
    return (2, 8, float(hash_uniform(seed, 16)[7]), seed)
