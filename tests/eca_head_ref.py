"""Reference of the pooling, ECA, layout, activation and mixture-head kernels of csrc/elementwise.hip and csrc/heads.hip, one
function per entry point, with the case tables and input generators of tests/test_eca_head_cpu.py and tests/test_eca_head_gpu.py.

Pure torch on the CPU.  Each function takes what its kernel takes and computes in the dtype it is handed: float64 is the
reference, float32 the plain CPU evaluation that the CPU test holds against the bounds of the GPU test.  Storage values (bfloat16 or
float32 activations) travel as float64 tensors that hold exactly representable values.  A sum comes with ``*_abs``, the sum of the
absolute values of the same terms, a stored value with ``mag``, the sum of the absolute values of its addends.  ``mut`` selects a
deliberately wrong variant (a mutant); tests/test_eca_head_cpu.py proves that every one of them is caught.

Bounds of the continuous kind (EPS24 = 2^-24, one float32 rounding of a value v is at most EPS24 |v|):
  sums      (L + 8) EPS24 sum|term|, L = the longest chain of sequential float32 additions of the launch
  stored    bfloat16: the rounded reference (generators leave nothing near a rounding boundary); float32: 8 EPS24 mag + EPS24 |ref|
  expf, expm1f, tanhf, logf: T_f units in the last place of the function's result (at most T_f 2^-23 |f|), carried through the
            arithmetic after the call by the reference's own derivative (``*_bounds`` functions below)

Device-library error, measured on gfx950 with this project's flags against float64 over dense sweeps (2^20 arguments per function,
2^12 for logf) by test_device_library_error_is_within_the_constants of tests/test_eca_head_gpu.py, which prints the figures and
holds them to the constants:
  expf    through pmoe_act_fwd(sigmoid), v in [-16, 0], err / (2^-23 y (1 - y)): includes the rounding of 1 + e and of the division
          (at most 2 units), and through pmoe_gate_mixture_bwd (dstd * expf(r), r in [-16, 0], one more rounding, 1/2 unit)
  expm1f  through pmoe_act_fwd(ELU), v in [-16, 0)
  tanhf   through pmoe_act_fwd(tanh), v in [-9, 9]
  logf    through pmoe_moe_loss at E = 1, z = 0, sigma_1 = 1: ll = -logf(sigma_0) - 2 * 0.9189..., sigma_0 in [2^-6, e^-2]
          (|log| in [2, 4.16]); the two subtractions add at most 1 unit
  measured worst, units in the last place:   expf 0.787 alone, 1.959 through the sigmoid   expm1f 0.866   tanhf 1.344   logf 2.633
  (none above 4).  T_f = twice the measured worst, rounded up to a whole unit, never below 1.

Left out on purpose: the grid-stride loops of maxpool_* and of the plain nchw_to_nhwc kernel (they need inputs of tens of millions
of elements) and the fp8 weight pack.  (The U-Net kernels of csrc/punet.hip, csrc/stage1.hip and csrc/stage0.hip: tests/unet_ref.py.)

act_bwd works from the SAVED output: with dropout an element whose saved output is zero counts as dropped (for tanh and ELU that
includes an input of exactly 0 that was kept); the reference follows the kernel's contract here, not torch's autograd.
"""
import functools
import math
import zlib

import numpy as np
import torch

from tests.bn_ref import EPS24, cdiv, chain_stream, partition, stream_geometry, ve  # noqa: F401
from tests.stem_tail_ref import BF16, F32, F64, bf16_boundary_distance, round_to  # noqa: F401

MEASURED = {"exp": 1.959, "expm1": 0.866, "tanh": 1.344, "log": 2.633}          # units in the last place, see the docstring
T_EXP, T_EXPM1, T_TANH, T_LOG = 4.0, 2.0, 3.0, 6.0                               # ceil(2 * measured)
ULP = 2.0 ** -23                     # one unit in the last place of v is at most ULP |v|
INF = float("inf")
DTYPES = (BF16, F32)
KINDS = ("lattice", "continuous")
ACT_NONE, ACT_RELU, ACT_ELU, ACT_TANH, ACT_SIGMOID = range(5)
LOSS_EPS = 2.0 ** -23
HALF_LOG_2PI = 0.9189385332046727


def tname(d):
    return "bf16" if d == BF16 else "f32"


def case_id(case):
    return "-".join(tname(v) if isinstance(v, torch.dtype) else str(v) for v in case)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def lat(g, shape, lim, den):
    """multiples of 1 / den in [-lim / den, lim / den]"""
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64) / den


def pick(g, shape, vals):
    return torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), shape, generator=g)]


def randn(g, shape, dtype=F32, scale=1.0):
    """randn in the storage type"""
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(F64)


def pow2(v):
    return v > 0 and not (v & (v - 1))


def pow2ceil(v):
    g = 1
    while g < v:
        g <<= 1
    return g


def near_boundary(v, margin, dtype):
    """v within ``margin`` of a rounding boundary of bfloat16 storage (float32 storage rounds nothing)"""
    if dtype != BF16:
        return torch.zeros_like(v, dtype=torch.bool)
    return (v != 0) & (bf16_boundary_distance(v.abs()) <= margin)


def settle(d, draw, ambiguous, tries=64):
    """redraw the elements that ``ambiguous`` (name -> mask over d[name]) marks until none is left"""
    for _ in range(tries):
        amb = ambiguous(d)
        if not any(m.any() for m in amb.values()):
            return d
        for n, m in amb.items():
            d[n] = torch.where(m, draw(n), d[n])
    raise AssertionError("ambiguous elements left after the redraws")


def again(v, mut):
    """the mutant that rounds a result to bfloat16 before it is stored (invisible in bfloat16 storage: it is tried in float32)"""
    return round_to(v, BF16).to(v.dtype) if mut == "round2" else v


def latw(g, shape, dtype):
    """multiples of 1/4 in the storage type: up to 2 in bfloat16, up to 512 (11 significant bits, more than bfloat16 holds) in
    float32, where a needless rounding to bfloat16 then shows"""
    return lat(g, shape, 8 if dtype == BF16 else 2048, 4)


def stored_bound(ref, mag, extra=0.0, L=0):
    """float32 storage: (L + 8) EPS24 mag + half a unit in the last place + a transcendental allowance"""
    return (L + 8) * EPS24 * mag + EPS24 * ref.abs() + extra


TOL = 2.0 ** -18                     # margin of the redraw rules, relative to mag: above (L + 8) EPS24 for L <= 56


# ---------------------------------------------------------------------------------------------------------------------------------
# launch geometry, from the launch code of csrc/elementwise.hip and csrc/heads.hip

def grid_stride_entered(nitems, cap):
    """grid_for(n, cap) launches min(ceil(n / 256), cap) workgroups of 256: the loop runs twice for some thread iff"""
    return cdiv(nitems, 256) > cap


GRID_CAPS = {"gap_bwd": 256, "eca_scale": 512, "eca_bwd_apply": 512, "pad_rows": 64, "gap_finish": 1024, "act": 4096}


def nhwc_route(B, C, H, W, Cp):
    """pmoe_nchw_to_nhwc: the kernel a shape takes"""
    HW = H * W
    if Cp <= 32 and cdiv(HW, 256) * B <= 0x7fffffff:
        return "tiled256"
    if Cp <= 240 and cdiv(HW, 64) * B <= 0x7fffffff:
        return "tiled64"
    return "plain"


def nhwc_tiles(HW, route):
    """(full tiles, pixels of the partial tile) per image"""
    pix = {"tiled256": 256, "tiled64": 64}.get(route)
    return (HW // pix, HW % pix) if pix else (0, 0)


def gate_G(E):
    return pow2ceil(E)


# ---------------------------------------------------------------------------------------------------------------------------------
# max pool 3x3, stride 2, pad 1

def pool_out(h):
    return (h + 2 - 3) // 2 + 1


def maxpool_fwd(x, mut=""):
    """maxpool_fwd_kernel: x [N, H, W, C] -> y and the tap 0..8 (row * 3 + col) of the FIRST maximum in scan order over the
    in-bounds taps (the first in-bounds tap is taken whatever it holds, -inf included)"""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    best = torch.full((N, Ho, Wo, C), -INF, dtype=x.dtype)
    am = torch.zeros((N, Ho, Wo, C), dtype=torch.int64)
    seen = torch.zeros(Ho, Wo, dtype=torch.bool)
    off = 0 if mut == "tap" else 1
    for r in range(3):
        for q in range(3):
            yy, xx = 2 * torch.arange(Ho) - off + r, 2 * torch.arange(Wo) - off + q
            ok = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
            v = x[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
            better = (v >= best) if mut == "last" else (v > best)
            take = ((ok & ~seen)[None, :, :, None] | better) & ok[None, :, :, None]
            best, am = torch.where(take, v, best), torch.where(take, torch.tensor(r * 3 + q), am)
            seen = seen | ok
    return {"y": best, "am": am.to(torch.uint8)}


def maxpool_bwd(dy, am, H, W, dtype, mut=""):
    """maxpool_bwd_kernel: dx[n, 2 oy - 1 + r, 2 ox - 1 + q, c] += dy[n, oy, ox, c] where am == r * 3 + q and the tap is in bounds;
    the sum of up to four gradients (exact in float32 for the generators' dy) is rounded once to the storage type"""
    N, Ho, Wo, C = dy.shape
    dx = torch.zeros(N, H, W, C, dtype=dy.dtype)
    off = 0 if mut == "tap" else 1
    for r in range(3):
        for q in range(3):
            yy, xx = 2 * torch.arange(Ho) - off + r, 2 * torch.arange(Wo) - off + q
            my, mx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
            c = torch.where(am == r * 3 + q, dy, torch.zeros((), dtype=dy.dtype))[:, my][:, :, mx]
            dx[:, yy[my][:, None], xx[mx][None, :]] += c
    return {"dx": round_to(dx, dtype)}


# (N, H, W, C in channel vectors, dtype)
MAXPOOL_CASES = [(n, h, w, cv * ve(d), d) for d in DTYPES for n, h, w, cv in (
    (1, 1, 2, 1),            # H = 1, W = 2: one output, taps above, below and left out of bounds
    (2, 2, 1, 1),            # W = 1
    (2, 5, 7, 8),            # odd x odd, several channel vectors
    (1, 4, 6, 1),            # even x even: the last window hangs over the edge by one
    (1, 8, 3, 64 // ve(d)),  # C = 64, more than one workgroup
    (3, 7, 4, 2))]           # odd x even


@functools.lru_cache(maxsize=None)
def maxpool_data(case, kind):
    """x: multiples of 1/4 (lattice: ties everywhere) or randn; in both kinds channel 1 mod 4 is ReLU'd (ties at 0), channel 2 mod 4
    holds -inf at a third of its pixels and window (0, 0) entirely, and planted windows hold two equal maxima / nine equal values.
    dy: multiples of 1/4, or randn rounded to bfloat16 with 2^-6 <= |dy| < 8, so that the sum of up to four of them is exact in
    float32: the forward pass rounds nothing, the backward pass once, to bfloat16 storage.  ``am_any``: arbitrary bytes 0..8 (out-of-bounds taps included)."""
    N, H, W, C, dtype = case
    g = gen("maxpool", case, kind)
    x = lat(g, (N, H, W, C), 8, 4) if kind == "lattice" else randn(g, (N, H, W, C), dtype)
    c = torch.arange(C)
    x[..., c % 4 == 1] = x[..., c % 4 == 1].clamp_min(0)
    hole = torch.rand(N, H, W, C, generator=g) < 1 / 3
    hole[:, :2, :2] = True
    x = torch.where(hole & (c % 4 == 2), torch.tensor(-INF, dtype=F64), x)
    if H >= 5 and W >= 3:
        x[:, 1, 1, 0::4], x[:, 2, 2, 0::4] = 5.0, 5.0            # window (1, 1): equal maxima at taps 0 and 4
        x[:, 3:6, 0:2, 3::4] = 7.0                               # window (2, 0): every in-bounds tap equal
    Ho, Wo = pool_out(H), pool_out(W)
    if kind == "lattice":
        dy = lat(g, (N, Ho, Wo, C), 8, 4)
    else:
        dy = randn(g, (N, Ho, Wo, C), BF16, 2.0)
        dy = torch.where(dy.abs() < 2.0 ** -6, torch.tensor(0.5, dtype=F64), dy).clamp(-7.5, 7.5)
    return {"x": x, "dy": dy, "am_any": torch.randint(0, 9, (N, Ho, Wo, C), generator=g).to(torch.uint8)}


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool

def gap_partial(a, b, nparts, b_ipe, mut=""):
    """gap_partial_kernel: part[n, p] = sum over partition p (bn_ref.partition) of image n's pixels of a, or of a * b[n % b_ipe]
    (b_ipe = 0: b[n])"""
    t = a
    if b is not None:
        idx = torch.arange(a.shape[0])
        if b_ipe > 0:
            idx = idx.clamp_max(b_ipe - 1) if mut == "share" else idx % b_ipe
        t = a * b[idx]
    t = t.reshape(t.shape[0], -1, t.shape[-1])
    s, ab = partition(t, nparts)
    if mut == "part":
        s = s.clone()
        s[:, (t.shape[1] - 1) // cdiv(t.shape[1], nparts)] = 0                  # the last partition that holds a pixel
    return {"part": s, "part_abs": ab}


# (E, ipe, H, W, C, dtype, nparts ("one" | "three" | "HW+2"), form ("a" | "ab" | "ab_shared"))
def _gap_partial_cases():
    out = []
    for d in DTYPES:
        v = ve(d)
        for cvs, h, w, parts, form in (
                (1, 7, 11, "three", "a"),          # CV = 1: 256 rows in flight; HW = 77 in 3 partitions of 26: ragged last one
                (1, 1, 1, "HW+2", "ab"),           # HW = 1, empty partitions
                (6, 7, 11, "three", "ab"),         # CV = 6 (48 bf16 channels): 256 % 6 = 4 idle lanes; private b
                (6, 7, 11, "one", "ab_shared"),    # shared b
                (6, 2, 3, "HW+2", "a"),            # more partitions than pixels
                (256, 3, 5, "three", "ab_shared"),  # CV = 256: RL = 1
                (256, 1, 2, "one", "a"),
                (8, 16, 16, "three", "ab_shared")):   # 256 pixels: 86 + 86 + 84
            out.append((2, 3, h, w, cvs * v, d, parts, form))
    return out


GAP_PARTIAL_CASES = _gap_partial_cases()


def nparts_of(name, hw):
    return {"one": 1, "three": 3, "HW+2": hw + 2}[name]


@functools.lru_cache(maxsize=None)
def gap_partial_data(case, kind):
    """a, b: multiples of 1/4 up to 2 (products: multiples of 1/16, sums of at most 256 of them below 2^10: exact), or randn"""
    E, ipe, H, W, C, dtype, parts, form = case
    g = gen("gap_partial", case, kind)
    N = E * ipe
    mk = (lambda s: lat(g, s, 8, 4)) if kind == "lattice" else (lambda s: randn(g, s, dtype))
    return {"a": mk((N, H, W, C)), "b": None if form == "a" else mk((ipe if form == "ab_shared" else N, H, W, C)),
            "b_ipe": ipe if form == "ab_shared" else 0}


def gap_finish(part, HW, dtype, mut=""):
    """gap_finish_kernel: out[n, c] = (sum_p part[n, p, c]) * (1 / HW), rounded to the storage type"""
    p = part[:, :-1] if mut == "part" else part
    s, sabs = p.sum(1), part.abs().sum(1)
    inv = torch.ones((), dtype=part.dtype) / (1 if mut == "nohw" else HW)
    return {"out": round_to(again(s * inv, mut), dtype), "raw": s * inv, "mag": sabs * inv}


# (N, C, nparts, HW, out_ld, out_coff, dtype); lattice needs a power-of-two HW (1 / HW exact)
GAP_FINISH_CASES = [c + (d,) for d in DTYPES for c in (
    (3, 64, 3, 16, 192, 64),           # a window in the middle of wider rows
    (2, 5, 1, 1, 16, 3),               # HW = 1, an odd window
    (2, 64, 3, 77, 64, 0),             # 1 / 77: continuous only
    (257, 1024, 1, 4, 1024, 0))]       # N * C = 263168 > 1024 * 256: the grid-stride loop


def kinds_of(hw):
    return KINDS if pow2(hw) else ("continuous",)


@functools.lru_cache(maxsize=None)
def gap_finish_data(case, kind):
    N, C, nparts, HW, ld, coff, dtype = case
    g = gen("gap_finish", case, kind)
    if kind == "lattice":
        return {"part": latw(g, (N, nparts, C), F32)}
    d = {"part": randn(g, (N, nparts, C), F32, HW ** 0.5)}

    def amb(d):
        r = gap_finish(d["part"], HW, dtype)
        return {"part": near_boundary(r["raw"], TOL * r["mag"], dtype)[:, None].expand_as(d["part"])}
    return settle(d, lambda n: randn(g, (N, nparts, C), F32, HW ** 0.5), amb)


def gap_bwd(gr, HW, C, coff, dtype, mut=""):
    """gap_bwd_kernel: dx[n, p, c] = g[n, coff + c] * (1 / HW) for every pixel p, rounded"""
    inv = torch.ones((), dtype=gr.dtype) / (1 if mut == "nohw" else HW)
    v = gr[:, coff:coff + C] * inv
    row = round_to(again(v, mut), dtype)
    return {"dx": row[:, None].expand(-1, HW, -1), "raw": v, "mag": v.abs()}


# (N, H, W, C, g_ld, g_coff, dtype)
GAP_BWD_CASES = [(2, 1, 1, 64, 64, 0, d) for d in DTYPES] + [(2, 4, 4, 64, 192, 64, d) for d in DTYPES] + \
                [(3, 3, 5, ve(d), 4 * ve(d), 2 * ve(d), d) for d in DTYPES] + [
    (1, 33, 32, 512, 512, 0, BF16),        # 1056 * 64 vectors > 256 * 256: the grid-stride loop (1 / 1056: continuous only)
    (1, 32, 64, 512, 1536, 512, BF16)]     # the same loop at a power-of-two HW, for the lattice


@functools.lru_cache(maxsize=None)
def gap_bwd_data(case, kind):
    N, H, W, C, ld, coff, dtype = case
    g = gen("gap_bwd", case, kind)
    if kind == "lattice":
        return {"g": latw(g, (N, ld), dtype)}
    d = {"g": randn(g, (N, ld), dtype)}

    def amb(d):
        r = gap_bwd(d["g"], H * W, C, coff, dtype)
        m = torch.zeros(N, ld, dtype=torch.bool)
        m[:, coff:coff + C] = near_boundary(r["raw"], TOL * r["mag"], dtype)
        return {"g": m}
    return settle(d, lambda n: randn(g, (N, ld), dtype), amb)


# ---------------------------------------------------------------------------------------------------------------------------------
# ECA

def _taps(src, wrow, k, pad, cr, sign):
    """out[n, c] = sum_j wrow[n, j] * src[n, c + sign * (j - pad)] over the taps that land in [0, cr); and the same of absolutes"""
    N, C = src.shape
    c = torch.arange(C)
    out, ab = torch.zeros_like(src), torch.zeros_like(src)
    for j in range(k):
        cc = c + sign * (j - pad)
        ok = ((cc >= 0) & (cc < cr)).to(src.dtype)
        t = wrow[:, j:j + 1] * src[:, cc.clamp(0, C - 1)] * ok
        out, ab = out + t, ab + t.abs()
    return out, ab


def eca_gate(part, HW, w, k, N, ipe, in_ipe, C, creal, mut=""):
    """eca_gate_kernel: gapmean[n, c] = (sum_p part[n or n % ipe, p, c]) / HW for c < creal, else 0;
    gate[n, c] = sigmoid(sum_j w[n // ipe, j] * gapmean[n, c + j - k // 2]) (taps inside [0, creal)) for c < creal, else 0"""
    n = torch.arange(N)
    ni = (n.clamp_max(part.shape[0] - 1) if mut == "share" else n % ipe) if in_ipe > 0 else n
    p = part[ni]
    pp = p[:, :-1] if mut == "part" else p
    cr = C if mut == "creal" else creal
    live = (torch.arange(C) < cr)[None]
    inv = torch.ones((), dtype=part.dtype) / (1 if mut == "nohw" else HW)
    zero = torch.zeros((), dtype=part.dtype)
    gm, gm_abs = torch.where(live, pp.sum(1) * inv, zero), torch.where(live, p.abs().sum(1) * inv, zero)
    wrow = w[n // ipe]
    pad = k // 2 + (1 if mut == "tap" else 0)
    z, _ = _taps(gm, wrow, k, pad, cr, 1)
    _, z_abs = _taps(gm_abs, wrow, k, pad, cr, 1)
    return {"gate": torch.where(live, torch.sigmoid(z), zero), "gapmean": gm, "gm_abs": gm_abs, "z": z, "z_abs": z_abs}


def eca_gate_bounds(ref, nparts, k):
    """gapmean: a sum of nparts terms, times 1 / HW.  z: k products of gapmean, each off by at most (nparts + 8) EPS24 of its
    absolute sum, added in a chain of k: (nparts + k + 16) EPS24 z_abs.  gate = 1 / (1 + expf(-z)): the derivative g (1 - g)
    carries dz and the T_EXP units of expf (e / (1 + e)^2 = g (1 - g)); the addition and the division round g twice."""
    g = ref["gate"]
    dz = (nparts + k + 16) * EPS24 * ref["z_abs"]
    return {"gapmean": (nparts + 8) * EPS24 * ref["gm_abs"], "gate": g * (1 - g) * (dz + T_EXP * ULP) + 8 * EPS24 * g}


def eca_scale(x, gate, x_ipe, dtype, mut=""):
    """eca_scale_kernel: y[n] = x[n or n % x_ipe] * gate[n], rounded"""
    n = torch.arange(gate.shape[0])
    nx = (n.clamp_max(x.shape[0] - 1) if mut == "share" else n % x_ipe) if x_ipe > 0 else n
    v = x[nx] * gate[:, None, None, :]
    return {"y": round_to(again(v, mut), dtype), "raw": v, "mag": v.abs()}


def eca_bwd_small(dot_part, gate, gapmean, w, k, ipe, C, creal, dgap_scale, mut=""):
    """eca_bwd_small_kernel + eca_bwd_dw_kernel: dpre[n, c] = (sum_p dot_part[n, p, c]) * g * (1 - g) for c < creal, else 0;
    dgap[n, c] = dgap_scale * sum_j w[j] * dpre[n, c - j + k // 2] for c < creal, else 0;
    dw[e, j] = sum over the expert's images and c < creal of dpre[n, c] * gapmean[n, c + j - k // 2]"""
    N = dot_part.shape[0]
    dt = dot_part.dtype
    pp = dot_part[:, :-1] if mut == "part" else dot_part
    cr = C if mut == "creal" else creal
    live = (torch.arange(C) < cr)[None]
    zero = torch.zeros((), dtype=dt)
    gg = gate * (1 - gate)
    dpre, dpre_abs = torch.where(live, pp.sum(1) * gg, zero), torch.where(live, dot_part.abs().sum(1) * gg.abs(), zero)
    wrow = w[torch.arange(N) // ipe]
    pad = k // 2 + (1 if mut == "tap" else 0)
    d, _ = _taps(dpre, wrow, k, pad, cr, -1)
    _, d_abs = _taps(dpre_abs, wrow, k, pad, cr, -1)
    scale = torch.tensor(dgap_scale, dtype=dt)
    gml = torch.where(live, gapmean, zero)            # the taps read gapmean inside [0, creal) only
    c = torch.arange(C)
    dw_img, dw_abs = torch.zeros(N, k, dtype=dt), torch.zeros(N, k, dtype=dt)
    for j in range(k):
        cc = c + j - pad
        ok = ((cc >= 0) & (cc < cr)).to(dt)
        dw_img[:, j] = (dpre * gml[:, cc.clamp(0, C - 1)] * ok).sum(1)
        dw_abs[:, j] = (dpre_abs * gml[:, cc.clamp(0, C - 1)].abs() * ok).sum(1)
    return {"dgap": torch.where(live, d * scale, zero), "dgap_abs": torch.where(live, d_abs * scale.abs(), zero),
            "dw": dw_img.reshape(-1, ipe, k).sum(1), "dw_abs": dw_abs.reshape(-1, ipe, k).sum(1), "dpre": dpre}


def eca_bwd_small_bounds(ref, nparts, k, ipe, C):
    """dpre: nparts additions and three roundings (1 - g and two products).  dgap: k products in a chain, one more for the scale.
    dw: a thread adds its ceil(C / 256) channels' terms, thread j folds the 256 lanes, eca_bwd_dw_kernel adds ipe images:
    L = ceil(C / 256) + 256 + ipe; the terms' own roundings (nparts + 3 <= 8 with |dot_part| for |sum|) are inside the 8"""
    L = cdiv(C, 256) + 256 + ipe
    return {"dgap": (nparts + k + 16) * EPS24 * ref["dgap_abs"], "dw": (L + 8) * EPS24 * ref["dw_abs"], "L": L}


def eca_bwd_apply(dy, gate, dgap, dtype, mut=""):
    """eca_bwd_apply_kernel: dx = dy * gate + dgap * (1 / HW), rounded"""
    HW = dy.shape[1] * dy.shape[2]
    inv = torch.ones((), dtype=dy.dtype) / (1 if mut == "nohw" else HW)
    a, b = dy * gate[:, None, None, :], (dgap * inv)[:, None, None, :]
    return {"dx": round_to(again(a + b, mut), dtype), "raw": a + b, "mag": a.abs() + b.abs()}


# (E, ipe, C, creal, k, nparts, HW, shared input); lattice needs a power-of-two HW
ECA_CASES = [
    (2, 3, 16, 12, 3, 3, 16, False),         # the stem's 12 real channels of 16
    (2, 3, 16, 12, 9, 1, 16, True),          # k = 9 over 12 channels: taps cross channel 0 and channel creal - 1 at once; shared
    (2, 3, 144, 138, 5, 3, 64, True),        # the PMoE stem
    (2, 3, 64, 64, 1, 1, 4, False),          # k = 1: no neighbours
    (2, 3, 512, 512, 5, 3, 16, False),       # C > 256: the c += 256 loops, two terms per thread in the dw fold
    (2, 3, 1024, 1000, 9, 3, 16, True),      # the largest C, creal < C beyond the first 256
    (1, 1, 64, 64, 3, 1, 77, False)]         # 1 / 77: continuous only
DGAP_FORMS = ("one", "1/HW", "null")


@functools.lru_cache(maxsize=None)
def eca_data(case, kind):
    """inputs of eca_gate (part, w) and of eca_bwd_small (dot_part, gate_in, gapmean_in, w_b).  The pad channels creal..C-1 of
    every input hold finite junk: the kernels must not let it through.
    lattice: part, dot_part, gapmean: multiples of 1/4; eca_gate: expert 0's weights are zero, the others' in {0, 128, 256} * HW, and
    part >= 0 with seven of ten channels all zero: z is 0 (gate = 1/2) or a multiple of 32 (expf(-z) < 2^-46: 1 + e = 1 in
    float32 whatever expf's last bits are, and 1 - e^-32 rounds to 1: gate = 1 exactly); eca_bwd_small: gate in
    {0, 1/4, 1/2, 3/4, 1}, w: multiples of 1/2 -- dpre: multiples of 2^-6 below 2, dgap: of 2^-7 below 2^6, dw terms: of 2^-8
    below 4, at most 2^12 of them: exact in float32"""
    E, ipe, C, creal, k, nparts, HW, shared = case
    g = gen("eca", case, kind)
    N, nin = E * ipe, ipe if shared else E * ipe
    if kind == "lattice":
        part = lat(g, (nin, nparts, C), 8, 4).abs() * (torch.rand(nin, 1, C, generator=g) < 0.3)
        w = pick(g, (E, k), [0.0, 128.0, 256.0]) * HW
        w[0] = 0
        return {"part": part, "w": w, "dot_part": lat(g, (N, nparts, C), 8, 4), "gate_in": pick(g, (N, C), [0, .25, .5, .75, 1]),
                "gapmean_in": lat(g, (N, C), 8, 4), "w_b": lat(g, (E, k), 4, 2)}
    w = randn(g, (E, k), F32, 0.5)
    return {"part": randn(g, (nin, nparts, C), F32, HW ** 0.5), "w": w, "dot_part": randn(g, (N, nparts, C), F32, HW ** 0.5),
            "gate_in": torch.sigmoid(randn(g, (N, C))).to(F32).to(F64), "gapmean_in": randn(g, (N, C)), "w_b": w}


# eca_scale: (E, ipe, H, W, C, shared x, dtype)
ECA_SCALE_CASES = [(2, 3, 2, 3, ve(d), s, d) for d in DTYPES for s in (False, True)] + \
                  [(2, 3, 5, 7, 64 * ve(d), True, d) for d in DTYPES] + [
    (1, 1, 40, 52, 512, False, BF16)]        # 2080 * 64 vectors > 512 * 256: the grid-stride loop


@functools.lru_cache(maxsize=None)
def eca_scale_data(case, kind):
    E, ipe, H, W, C, shared, dtype = case
    g = gen("eca_scale", case, kind)
    N, nx = E * ipe, ipe if shared else E * ipe
    if kind == "lattice":
        return {"x": latw(g, (nx, H, W, C), dtype), "gate": pick(g, (N, C), [0, .25, .5, 1, 2, -1])}
    d = {"x": randn(g, (nx, H, W, C), dtype), "gate": torch.sigmoid(randn(g, (N, C))).to(F32).to(F64)}

    def amb(d):
        r = eca_scale(d["x"], d["gate"], ipe if shared else 0, dtype)
        m = near_boundary(r["raw"], TOL * r["mag"], dtype)
        return {"x": m.reshape(E, ipe, H, W, C).any(0) if shared else m}
    return settle(d, lambda n: randn(g, (nx, H, W, C), dtype), amb)


# eca_bwd_apply: (N, H, W, C, dtype)
ECA_APPLY_CASES = [(6, 2, 2, ve(d), d) for d in DTYPES] + [(2, 4, 4, 64 * ve(d), d) for d in DTYPES] + \
                  [(3, 5, 7, 64, d) for d in DTYPES] + [(1, 40, 52, 512, BF16), (1, 64, 64, 512, BF16)]


@functools.lru_cache(maxsize=None)
def eca_apply_data(case, kind):
    """lattice: dy * gate: multiples of 1/16 up to 4, dgap / HW: multiples of 1 / (4 HW) with HW <= 2^12: 18 bits, exact"""
    N, H, W, C, dtype = case
    g = gen("eca_apply", case, kind)
    if kind == "lattice":
        return {"dy": latw(g, (N, H, W, C), dtype), "gate": pick(g, (N, C), [0, .25, .5, .75, 1]), "dgap": lat(g, (N, C), 8, 4)}
    d = {"dy": randn(g, (N, H, W, C), dtype), "gate": torch.sigmoid(randn(g, (N, C))).to(F32).to(F64),
         "dgap": randn(g, (N, C), F32, H * W)}

    def amb(d):
        r = eca_bwd_apply(d["dy"], d["gate"], d["dgap"], dtype)
        return {"dy": near_boundary(r["raw"], TOL * r["mag"], dtype)}
    return settle(d, lambda n: randn(g, (N, H, W, C), dtype), amb)


# ---------------------------------------------------------------------------------------------------------------------------------
# layout

def nchw_to_nhwc(src, Cp, dtype, mut=""):
    """src f32 [B, C, H, W] -> [B, H, W, Cp], rounded once; pad channels +0"""
    B, C, H, W = src.shape
    out = torch.zeros(B, H, W, Cp, dtype=F64)
    s = src.roll(1, 1) if mut == "tap" else src                      # (the mutant: channel planes off by one)
    out[..., :C] = round_to(s.permute(0, 2, 3, 1), dtype)
    return {"dst": again(out, mut)}


def _nhwc_cases():
    out = []
    for cps, hws in (((16, 32), ((7, 9), (16, 16), (1, 257), (20, 30))), ((48, 240), ((7, 9), (8, 8), (5, 13), (10, 20))),
                     ((256,), ((7, 10),))):
        for cp in cps:
            for h, w in hws:
                for d in DTYPES:
                    out += [(1, cp, h, w, cp, d), (3, cp - 3 - (cp == 16), h, w, cp, d)]     # C = Cp, B = 1; C < Cp, B = 3
    return out


NHWC_CASES = _nhwc_cases()          # (B, C, H, W, Cp, dtype): Cp <= 32 at HW 63 | 256 | 257 | 600, Cp <= 240 at 63 | 64 | 65 | 200, Cp = 256


@functools.lru_cache(maxsize=None)
def nhwc_data(case, kind):
    B, C, H, W, Cp, dtype = case
    g = gen("nhwc", case, kind)
    src = latw(g, (B, C, H, W), F32) if kind == "lattice" else randn(g, (B, C, H, W), F32)
    src[0, 0, 0, 0] = -0.0
    return {"src": src}


def pad_rows(src, Kp, dtype):
    """src f32 [B, K] -> [B, Kp], rounded once; pad columns +0"""
    out = torch.zeros(src.shape[0], Kp, dtype=F64)
    out[:, :src.shape[1]] = round_to(src, dtype)
    return {"dst": out}


# (B, K, Kp, dtype)
PAD_ROWS_CASES = [c + (d,) for d in DTYPES for c in ((5, 16, 16), (5, 1, 16), (3, 6, 16), (257, 6, 64))]   # 257 * 64 > 64 * 256


# ---------------------------------------------------------------------------------------------------------------------------------
# activation + inverted dropout

def hash_uniform(seed, n):
    """hash_uniform(seed, 0..n-1) of csrc/common.h in 64-bit integer arithmetic: a float32 multiple of 2^-24 in [0, 1)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return torch.from_numpy((z >> np.uint64(40)).astype(np.int64)).to(F64) / 16777216.0


def keep_mask(n, drop_p, seed, mut=""):
    """kept iff hash >= drop_p as float32"""
    if not drop_p > 0:
        return torch.ones(n, dtype=torch.bool)
    u = hash_uniform(seed, n + 1)
    u = u[1:] if mut == "tap" else u[:n]
    p = torch.tensor(drop_p, dtype=F32).to(F64)
    return (u > p) if mut == "last" else (u >= p)


def keep_scale(drop_p, dt):
    """1.f / (1.f - drop_p) in float32 arithmetic"""
    if not drop_p > 0:
        return torch.ones((), dtype=dt)
    p = torch.tensor(drop_p, dtype=F32)
    return (1 / (1 - p)).to(dt)


def act_apply(act, v):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def act_fwd(x, act, drop_p, seed, dtype, mut=""):
    """act_fwd_kernel: y = kept ? act(x) * keep_scale : 0, rounded.  ``allow``: the transcendental allowance of the float32
    value: T_EXPM1 units of expm1f, T_TANH of tanhf, T_EXP of expf through y (1 - y) plus two roundings of y"""
    v = act_apply(act, x)
    ks = keep_scale(drop_p, x.dtype)
    keep = keep_mask(x.numel(), drop_p, seed, mut).reshape(x.shape)
    allow = {ACT_ELU: T_EXPM1 * ULP * torch.where(x > 0, torch.zeros_like(v), v.abs()), ACT_TANH: T_TANH * ULP * v.abs(),
             ACT_SIGMOID: T_EXP * ULP * v * (1 - v) + 2 * EPS24 * v.abs()}.get(act, torch.zeros_like(v))
    raw = torch.where(keep, v * ks, torch.zeros((), dtype=x.dtype))
    return {"y": round_to(again(raw, mut), dtype), "raw": raw, "mag": raw.abs(), "keep": keep, "allow": torch.where(keep, allow * ks, 0 * allow)}


def act_bwd(dy, y, act, drop_p, dtype, mut=""):
    """act_bwd_kernel, from the saved output y: with u = y / keep_scale
    none: dy * keep_scale (0 where dropout is on and y == 0); relu: y > 0 ? dy * keep_scale : 0;
    else 0 where dropout is on and y == 0, dy * f'(u) * keep_scale with f' = u > 0 ? 1 : u + 1 | 1 - u^2 | u (1 - u)"""
    ks = keep_scale(drop_p, dy.dtype)
    zero = torch.zeros((), dtype=dy.dtype)
    dropped = (y == 0) & (drop_p > 0) if mut != "last" else torch.zeros_like(y, dtype=torch.bool)
    if act == ACT_NONE:
        raw = torch.where(dropped, zero, dy * ks)
        mag = raw.abs()
    elif act == ACT_RELU:
        raw = torch.where(y > 0, dy * ks, zero)
        mag = raw.abs()
    else:
        u = y * (1 / ks)
        if mut == "tap":
            u = y
        if act == ACT_ELU:
            dv, dm = torch.where(u > 0, torch.ones_like(u), u + 1), torch.where(u > 0, torch.ones_like(u), u.abs() + 1)
        elif act == ACT_TANH:
            dv, dm = 1 - u * u, 1 + u * u
        else:
            dv, dm = u * (1 - u), (u * (1 - u)).abs()            # (1 - u rounds relative to itself)
        raw, mag = torch.where(dropped, zero, dy * dv * ks), torch.where(dropped, zero, (dy * dm * ks).abs())
    return {"dx": round_to(again(raw, mut), dtype), "raw": raw, "mag": mag}


BIG_ACT_N = (4096 * 256 + 3) * 4            # float32 vectors: more than 4096 workgroups of 256
SEEDS = (5, (1 << 40) + 12345)
# (n, act, drop_p, seed, dtype)
ACT_CASES = [(nv * ve(d), a, p, s, d) for d in DTYPES for a in range(5) for nv in (1, 300) for p, s in ((0.0, 0), (0.5, SEEDS[0]))] + \
            [(300 * ve(d), a, 0.5, SEEDS[1], d) for d in DTYPES for a in (ACT_NONE, ACT_ELU)] + \
            [(BIG_ACT_N, ACT_ELU, 0.5, SEEDS[1], F32)]


@functools.lru_cache(maxsize=None)
def act_data(case, kind):
    """lattice: x = multiples of 1/4 (none, relu), 0 and positive multiples (ELU), 0 (tanh, sigmoid: f(0) is exact); the saved
    output of act_bwd: multiples of 1/4 inside the function's range times keep_scale, zeros among them; dy: multiples of 1/4.
    continuous: randn * 2, redrawn where the stored bfloat16 value could round the other way; act_bwd gets the reference's y."""
    n, act, p, seed, dtype = case
    g = gen("act", case, kind)
    ks = 2.0 if p > 0 else 1.0
    if kind == "lattice":
        x = latw(g, (n,), dtype)
        x = x.abs() * (torch.rand(n, generator=g) < 0.7) if act == ACT_ELU else x * 0 if act in (ACT_TANH, ACT_SIGMOID) else x
        ysav = {ACT_NONE: lat(g, (n,), 8, 4), ACT_RELU: lat(g, (n,), 8, 4).clamp_min(0), ACT_ELU: lat(g, (n,), 8, 4).clamp_min(-0.75),
                ACT_TANH: lat(g, (n,), 3, 4), ACT_SIGMOID: pick(g, (n,), [0.25, 0.5, 0.75])}[act] * ks
        if p > 0:
            ysav = ysav * (torch.rand(n, generator=g) < 0.5)
        return {"x": x, "y": ysav, "dy": latw(g, (n,), dtype)}
    d = {"x": randn(g, (n,), dtype, 2.0), "dy": randn(g, (n,), dtype)}

    def amb(d):
        r = act_fwd(d["x"], act, p, seed, dtype)
        m = near_boundary(r["raw"], TOL * r["mag"] + 2 * r["allow"], dtype)
        y = r["y"]
        b = act_bwd(d["dy"], y, act, p, dtype)
        # (the saved output is bfloat16 here: f'(u) is exact in float32 and only the two products round, relative to the result)
        return {"x": m, "dy": near_boundary(b["raw"], TOL * b["raw"].abs(), dtype) & ~m}
    d = settle(d, lambda nm: randn(g, (n,), dtype, 2.0 if nm == "x" else 1.0), amb)
    d["y"] = act_fwd(d["x"], act, p, seed, dtype)["y"]
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# mixture head

def head_ld_of(E, shared):
    """row length of the head buffer in the tests: the used columns and three pad columns, in whole 8-element groups"""
    return cdiv((5 * E if shared else 5) + 3, 8) * 8


SPD_LD = 4


def head_views(head, B, E, shared):
    """comp [B, E, 4] (mean0, mean1, rawstd0, rawstd1), alpha [B, E] of either head layout"""
    if shared:
        return head[:B, :4 * E].reshape(B, E, 4), head[:B, 4 * E:5 * E]
    h = head[:E * B].reshape(E, B, -1).permute(1, 0, 2)
    return h[..., :4], h[..., 4]


def gate_fwd(head, spd, B, E, alpha_relu, shared, mut=""):
    """gate_fwd_kernel: probs = softmax over the E experts of alpha (relu'd if alpha_relu & 1; alpha itself if alpha_relu & 2),
    mean = the two mean columns, std = elu(rawstd) + 1, speeds = column 0 of spd: [B, E, 1], or [B, 1] in the shared layout"""
    comp, alpha = head_views(head, B, E, shared)
    a = alpha.clamp_min(0) if alpha_relu & 1 else alpha
    G = gate_G(E)
    if alpha_relu & 2:
        probs, pb = a.clone(), torch.zeros_like(a)
    else:
        m = a.max(1, keepdim=True).values
        if mut == "G" and G > E:
            m = m.clamp_min(0)
        ex = torch.exp(a - m)
        s = ex.sum(1, keepdim=True) + ((G - E) * torch.exp(-m) if mut == "G" else 0)
        probs = ex / s
        # two expf (numerator, and the denominator's weighted mean of them), the rounding of a - m on both sides, log2 G additions
        # of the butterfly, the division
        pb = probs * (2 * T_EXP * ULP + (math.log2(G) + 8) * EPS24 + 2 * EPS24 * (a - m).abs().max(1, keepdim=True).values)
    r = comp[..., 2:4]
    sd = torch.where(r > 0, r, torch.expm1(r)) + 1
    sdb = EPS24 * sd.abs() + torch.where(r > 0, torch.zeros_like(r), T_EXPM1 * ULP * torch.expm1(r).abs())
    speeds = spd[:B, 0:1] if shared else spd[:E * B, 0].reshape(E, B).t()[..., None]
    return {"probs": probs, "probs_bound": pb, "mean": comp[..., 0:2].contiguous(), "std": sd, "std_bound": sdb,
            "speeds": speeds.contiguous()}


def gate_bwd(head, probs, dprobs, dmean, dstd, dspeeds, B, E, alpha_relu, shared, rows, ld, spd_ld, dtype, mut=""):
    """gate_bwd_kernel: dalpha = p (dp - sum_e p dp) (dp itself in the raw mode), zero where alpha_relu & 1 and alpha <= 0;
    dmean copied; drawstd = dstd * (raw > 0 ? 1 : exp(raw)); pad columns of dhead and columns >= 1 of dspd zero; a null gradient
    counts as zeros.  ``rows``: the rows of the buffers (rows beyond the layout's stay untouched: NaN here)"""
    dt = probs.dtype
    comp, alpha = head_views(head, B, E, shared)
    z2, z1 = torch.zeros(B, E, 2, dtype=dt), torch.zeros(B, E, dtype=dt)
    dp = z1 if dprobs is None else dprobs
    dm, ds = z2 if dmean is None else dmean, z2 if dstd is None else dstd
    dot, dot_abs = (probs * dp).sum(1, keepdim=True), (probs * dp).abs().sum(1, keepdim=True)
    if mut == "G":
        dot = dot * 0
    da, da_mag = (dp, dp.abs()) if alpha_relu & 2 else (probs * (dp - dot), probs.abs() * (dp.abs() + dot_abs))
    if alpha_relu & 1 and mut != "last":
        keep = alpha > 0
        da, da_mag = torch.where(keep, da, 0 * da), torch.where(keep, da_mag, 0 * da_mag)
    r = comp[..., 2:4]
    f = torch.where(r > 0, torch.ones_like(r), torch.exp(r))
    dr = ds * f
    allow_r = torch.where(r > 0, torch.zeros_like(r), T_EXP * ULP * dr.abs())
    vals = torch.cat([dm, dr, da[..., None]], -1)                      # [B, E, 5]
    mags = torch.cat([dm.abs(), dr.abs(), da_mag[..., None]], -1)
    allow = torch.cat([0 * dm, allow_r, 0 * da[..., None]], -1)
    nan = float("nan")
    out = {}
    for name, src in (("dhead", vals), ("mag", mags), ("allow", allow)):
        t = torch.full((rows, ld), nan if name == "dhead" else 0.0, dtype=dt)
        if shared:
            t[:B] = 0
            t[:B, :4 * E] = src[..., :4].reshape(B, 4 * E)
            t[:B, 4 * E:5 * E] = src[..., 4]
        else:
            t[:E * B] = 0
            t[:E * B, :5] = src.permute(1, 0, 2).reshape(E * B, 5)
        out[name] = t
    dspd = torch.full((rows, spd_ld), nan, dtype=dt)
    nr = B if shared else E * B
    dspd[:nr] = 0
    if dspeeds is not None:
        dspd[:nr, 0] = dspeeds.reshape(B) if shared else dspeeds.reshape(B, E).t().reshape(-1)
    out["dhead_raw"] = out["dhead"]
    out["dhead"], out["dspd"] = round_to(again(out["dhead_raw"], mut), dtype), round_to(dspd, dtype)
    return out


def _gate_cases():
    out = []
    for E in (1, 3, 8, 33, 64):
        G = gate_G(E)
        for B in sorted({1, 5, 256 // G + 1}):             # 256 / G + 1: one sample more than a workgroup holds
            for ar in ((0, 2, 3) if E == 1 else (0, 1)):   # E = 1: plain, raw, raw + relu
                for shared in (False, True):
                    for d in DTYPES:
                        if B > 5 and (d == F32) == shared:         # the large batches once per layout
                            continue
                        out.append((E, B, ar, shared, d))
    out += [(3, 5, 3, False, BF16), (33, 5, 2, True, F32)]          # the raw mode with several experts: the lattice of E = 3, 33
    return out


GATE_CASES = _gate_cases()          # (E, B, alpha_relu, shared, dtype)
GATE_NULLS = ("none", "dprobs", "dmean", "dstd", "dspeeds")


def gate_kinds(case):
    return KINDS


@functools.lru_cache(maxsize=None)
def gate_data(case, kind):
    """head, spd in the storage type, two rows more than the layout has.  alpha: planted at 0 and one step either side in a third
    of the elements.  lattice: means and gradients multiples of 1/4, raw std in {0, 1/4, 1/2, 1, 2} (std = raw + 1, exp(0) = 1),
    softmax (E > 1, not the raw mode): without the ReLU and with a power-of-two E a sample's alphas are equal (probs = 1 / E);
    else a power-of-two number of the sample's experts (half of pow2ceil(E)) share one alpha and the others lie 256 or more
    below -- with the ReLU: {256, 258, 260} against |alpha| <= 2, the planted ones among them; without: 0 against -256, -258,
    -260 -- so that expf(alpha - max) is 1 or underflows to 0, probs = 1 / count or 0 exactly, and the reference's 1e-111 rounds
    to 0; the probabilities handed to gate_bwd: multiples of 1/8 in [0, 1]
    (p dp: multiples of 2^-5, their sum over <= 64 experts below 2^7, p (dp - dot): multiples of 2^-8 below 2^8: exact)."""
    E, B, ar, shared, dtype = case
    g = gen("gate", case, kind)
    ld = head_ld_of(E, shared)
    rows = (B if shared else E * B) + 2
    step = 0.25 if kind == "lattice" else 2.0 ** -7
    plant = pick(g, (B, E), [0.0, step, -step])
    if kind == "lattice":
        head, spd = lat(g, (rows, ld), 8, 4), lat(g, (rows, SPD_LD), 8, 4)
        raw, alpha = pick(g, (B, E, 2), [0, .25, .5, 1, 2]), lat(g, (B, E), 8, 4)
        alpha = torch.where(torch.rand(B, E, generator=g) < 1 / 3, plant, alpha)
        if not ar & 2 and E > 1:
            if not ar & 1 and pow2(E):
                alpha = alpha[:, :1].expand(B, E)
            else:
                live = torch.argsort(torch.rand(B, E, generator=g), 1) < pow2ceil(E) // 2     # a permutation: that many are below
                far = pick(g, (B, E), [256.0, 258.0, 260.0])
                alpha = torch.where(live, far[:, :1].expand(B, E), alpha) if ar & 1 else torch.where(live, 0 * far, -far)
        probs_in = torch.randint(0, 9, (B, E), generator=g).to(F64) / 8
        mk = lambda s: lat(g, s, 8, 4)
    else:
        head, spd = randn(g, (rows, ld), dtype), randn(g, (rows, SPD_LD), dtype)
        comp, alpha = head_views(head, B, E, shared)
        raw = comp[..., 2:4].clone()
        raw[..., 0] = torch.where(torch.rand(B, E, generator=g) < 0.2, torch.zeros(()).to(F64), raw[..., 0])      # raw == 0: the ELU edge
        alpha = torch.where(torch.rand(B, E, generator=g) < 1 / 3, plant, alpha)
        probs_in = torch.softmax(randn(g, (B, E)), 1).to(F32).to(F64)
        mk = lambda s: randn(g, s)
    comp, _ = head_views(head, B, E, shared)
    full = torch.cat([comp[..., :2], raw, alpha[..., None]], -1)
    if shared:
        head[:B, :4 * E], head[:B, 4 * E:5 * E] = full[..., :4].reshape(B, 4 * E), full[..., 4]
    else:
        head[:E * B, :5] = full.permute(1, 0, 2).reshape(E * B, 5)
    d = {"head": head, "spd": spd, "probs": probs_in, "dprobs": mk((B, E)), "dmean": latw(g, (B, E, 2), dtype) if kind == "lattice" else mk((B, E, 2)), "dstd": mk((B, E, 2)),
         "dspeeds": mk((B, 1) if shared else (B, E, 1)), "rows": rows, "ld": ld}
    if kind == "continuous" and dtype == BF16:
        def amb(d):
            r = gate_bwd(d["head"], d["probs"], d["dprobs"], d["dmean"], d["dstd"], d["dspeeds"], B, E, ar, shared, rows, ld, SPD_LD, dtype)
            m = near_boundary(torch.nan_to_num(r["dhead_raw"]), TOL * r["mag"] + 2 * r["allow"], dtype)
            c, a_ = head_views(m, B, E, shared)
            # the gradient that feeds an ambiguous element is redrawn (a row's dalpha depends on every dprobs of the row)
            return {"dmean": c[..., :2].clone(), "dstd": c[..., 2:4].clone(), "dprobs": a_.any(1, keepdim=True).expand(B, E).clone()}
        d = settle(d, lambda n: randn(g, tuple(d[n].shape)), amb)
        # (the gradients are float32 on the device; what is stored in bfloat16 is dhead.  dmean and dspeeds are stored rounded once.)
    return d


def moe_loss(probs, mean, sd, speeds, act, tgt, c0, c1, B, E, shared_speed, mut=""):
    """moe_loss_kernel, MixtureSameFamily.log_prob written out:
      pn = p / sum p, l = log(clamp(pn, eps, 1 - eps)), eps = 2^-23, lsm = log_softmax(l)
      comp_e = sum_d -(a_d - mu_ed)^2 / (2 sigma_ed^2) - log sigma_ed - log(2 pi) / 2,   ll_b = logsumexp_e(comp_e + lsm_e)
      loss = c0 * mean_b(-ll_b) + c1 * mean((speed - target)^2) [/ E over [B, E, 1] speeds]
    with r = exp(comp + lsm - ll), q = exp(lsm), gs = -c0 / B:
      dprobs = gs (r - q) / p, zero where the clamp is active; dmean = gs r (a - mu) / sigma^2;
      dstd = gs r ((a - mu)^2 / sigma^3 - 1 / sigma); dspeeds = 2 c1 (speed - target) / B [/ E^2]"""
    dt = probs.dtype
    a = act[:, None, :]
    diff = a - mean
    z = diff / sd
    logsd = torch.log(sd)
    comp = (-0.5 * z * z - logsd - HALF_LOG_2PI).sum(-1)
    ps = probs.sum(1, keepdim=True)
    pn = probs / ps
    clamped = (pn < LOSS_EPS) | (pn > 1 - LOSS_EPS)
    l = torch.log(pn.clamp(LOSS_EPS, 1 - LOSS_EPS))
    lse_l = torch.logsumexp(l, 1, keepdim=True)
    lsm = l - lse_l
    t = comp + lsm
    ll = torch.logsumexp(t, 1)
    r, q = torch.exp(t - ll[:, None]), torch.exp(lsm)
    gs = torch.tensor(-c0, dtype=dt) / B
    dprobs = gs * (r - q) / (pn * ps)
    if mut != "clampgrad":
        dprobs = torch.where(clamped, torch.zeros((), dtype=dt), dprobs)
    iv = 1 / (sd * sd)
    dmean = gs * r[..., None] * diff * iv
    A, Bt = diff * diff * iv / sd, 1 / sd
    dstd = gs * r[..., None] * (A - Bt)
    dsp = speeds - (tgt[:, None] if shared_speed else tgt[:, None, None])
    den = B if shared_speed else B * E * E
    if mut == "nohw":
        den = B
    dspeeds = torch.tensor(c1, dtype=dt) * 2 * dsp / den
    mse = (dsp * dsp).sum()
    loss = torch.tensor(c0, dtype=dt) * (-ll).sum() / B + torch.tensor(c1, dtype=dt) * mse / den
    return {"loss": loss.reshape(1), "loglik": ll, "dprobs": dprobs, "dmean": dmean, "dstd": dstd, "dspeeds": dspeeds,
            "clamped": clamped, "pn": pn,
            "_": dict(z=z, diff=diff, logsd=logsd, comp=comp, l=l, lse_l=lse_l, lsm=lsm, t=t, r=r, q=q, gs=gs, iv=iv, A=A, Bt=Bt,
                      dsp=dsp, den=den, mse=mse, a=a, ps=ps)}


def moe_loss_bounds(ref, probs, mean, sd, speeds, act, tgt, c0, c1, B, E, shared_speed):
    """Error bounds of moe_loss_kernel against ``ref`` (float64), step by step; u = EPS24, U_f = T_f 2^-23, G = pow2ceil(E).
      z = (a - mu) / sigma:            dz = u ((|a| + |mu|) / sigma + |z|)
      comp: per d, -z^2 / 2 off by |z| dz + u z^2, logf(sigma) by U_log |log sigma|, six additions of at most the absolute sum
            M = sum_d (z^2 / 2 + |log sigma| + log(2 pi) / 2):    dcomp = sum_d (|z| dz + U_log |log sigma|) + 8 u M
      pn = p / sum p: log2 G additions and a division, relative (log2 G + 2) u; l = logf(.):   dl = (log2 G + 2) u + U_log |l|
      ls = sum exp(l - lm): relative dLS = 2 max dl + u max|l - lm| + U_exp + log2 G u;   log ls: dLS + U_log |log ls|
      lsm = l - (lm + log ls):         dlsm = dl + max dl + dLS + U_log |log ls| + 2 u (|l| + |lm| + |log ls|)
      t = comp + lsm:                  dt = dcomp + dlsm + u (|comp| + |lsm|)
      ll = tm + logf(sum exp(t - tm)): dll = 3 max dt + u max|t - tm| + U_exp + log2 G u + U_log |log ts| + 2 u (|tm| + |log ts|)
      r = exp(t - ll): dr = r (dt + dll + u |t - ll| + U_exp);   q = exp(lsm): dq = q (dlsm + U_exp)
      dprobs = gs (r - q) / p:         |gs| (dr + dq + u (r + q)) / p + 6 u |dprobs|
      dmean  = gs r (a - mu) iv:       |gs| iv (dr |a - mu| + u r (|a| + |mu|)) + 8 u |dmean|
      dstd   = gs r (A - 1 / sigma):   |gs| (dr |A - 1 / sigma| + r (2 u (|a| + |mu|) |a - mu| iv / sigma + 8 u (A + 1 / sigma))) + 2 u |dstd|
      dspeeds: 2 |c1| u (|speed| + |target|) / den + 6 u |dspeeds|
      loss: a thread adds ceil(B / (256 / G)) samples, then an 8-level tree: L = ceil(B G / 256) + 8;
            |c0| / B (sum dll + (L + 8) u sum|ll|) + |c1| / den (sum 2 |ds| u (|speed| + |target|) + (L + 8) u sum ds^2) + 4 u (|both terms|)
    The gradients that carry a responsibility r get 2^-126 more: below it float32 underflows."""
    u, Ue, Ul = EPS24, T_EXP * ULP, T_LOG * ULP
    k = ref["_"]
    lg = math.log2(gate_G(E))
    mx = lambda v: v.max(1, keepdim=True).values
    amu = k["a"].abs() + mean.abs()
    dz = u * (amu / sd + k["z"].abs())
    M = (0.5 * k["z"] ** 2 + k["logsd"].abs() + HALF_LOG_2PI).sum(-1)
    dcomp = (k["z"].abs() * dz + u * k["z"] ** 2 + Ul * k["logsd"].abs()).sum(-1) + 8 * u * M
    l, lm = k["l"], mx(k["l"])
    dl = (lg + 2) * u + Ul * l.abs()
    logls = k["lse_l"] - lm
    dLS = 2 * mx(dl) + u * mx((l - lm).abs()) + Ue + lg * u
    dlsm = dl + mx(dl) + dLS + Ul * logls.abs() + 2 * u * (l.abs() + lm.abs() + logls.abs())
    dt = dcomp + dlsm + u * (k["comp"].abs() + k["lsm"].abs())
    t, tm = k["t"], mx(k["t"])
    logts = ref["loglik"][:, None] - tm
    dll = 3 * mx(dt) + u * mx((t - tm).abs()) + Ue + lg * u + Ul * logts.abs() + 2 * u * (tm.abs() + logts.abs())
    r, q, gs = k["r"], k["q"], k["gs"].abs()
    dr = r * (dt + dll + u * (t - ref["loglik"][:, None]).abs() + Ue)
    dq = q * (dlsm + Ue)
    out = {"loglik": dll[:, 0]}
    out["dprobs"] = torch.where(ref["clamped"], torch.zeros_like(r), gs * (dr + dq + u * (r + q)) / probs + 6 * u * ref["dprobs"].abs())
    out["dmean"] = gs * k["iv"] * (dr[..., None] * k["diff"].abs() + u * r[..., None] * amu) + 8 * u * ref["dmean"].abs()
    out["dstd"] = gs * (dr[..., None] * (k["A"] - k["Bt"]).abs()
                        + r[..., None] * (2 * u * amu * k["diff"].abs() * k["iv"] / sd + 8 * u * (k["A"] + k["Bt"]))) + 2 * u * ref["dstd"].abs()
    tg = tgt[:, None] if shared_speed else tgt[:, None, None]
    smag = speeds.abs() + tg.abs()
    out["dspeeds"] = 2 * abs(c1) * u * smag / k["den"] + 6 * u * ref["dspeeds"].abs()
    L = cdiv(B * gate_G(E), 256) + 8
    nll_b = abs(c0) / B * (dll.sum() + (L + 8) * u * ref["loglik"].abs().sum())
    mse_b = abs(c1) / k["den"] * ((2 * k["dsp"].abs() * u * smag).sum() + (L + 8) * u * k["mse"])
    for n in ("dprobs", "dmean", "dstd"):                # float32 underflow: a responsibility below 2^-126 is flushed or denormal
        out[n] = torch.where(ref["clamped"], out[n], out[n] + 2.0 ** -126) if n == "dprobs" else out[n] + 2.0 ** -126
    out["loss"] = (nll_b + mse_b + 4 * u * (abs(c0) * ref["loglik"].abs().sum() / B + abs(c1) * k["mse"] / k["den"])).reshape(1)
    return out


# (E, B, shared_speed)
LOSS_CASES = [(E, B, s) for E in (1, 3, 8, 33, 64) for B in sorted({1, 5, 256 // gate_G(E) + 1}) for s in (False, True)]
LOSS_C = (0.75, 0.25)


@functools.lru_cache(maxsize=None)
def loss_data(case, kind):
    """continuous: float32 probabilities (softmax of randn, not renormalised after rounding), means, std = elu + 1 of randn,
    actions in [-1, 1], targets in [0, 1]; with E > 1 row 0 has one probability of 2^-30 (the lower clamp, zero dprobs there) and
    no other normalised probability is within a factor 2^10 of the clamp at 2^-23 or above 1 - 2^-10; E = 1: p / p = 1 is clamped
    from above.  lattice (c0 = 0: the speed branch alone): speeds and targets multiples of 1/4, c1 = 1/2; exact where the
    denominator B (shared) or B E^2 is a power of two."""
    E, B, shared = case
    g = gen("loss", case, kind)
    probs = torch.softmax(randn(g, (B, E)) * 1.5, 1).clamp_min(2.0 ** -12).to(F32).to(F64)
    if E > 1:
        probs[0, E - 1] = 2.0 ** -30
    raw = randn(g, (B, E, 2))
    sd = (torch.where(raw > 0, raw, torch.expm1(raw)) + 1).to(F32).to(F64)
    d = {"probs": probs, "mean": randn(g, (B, E, 2)), "std": sd, "act": (torch.rand(B, 2, generator=g) * 2 - 1).to(F32).to(F64),
         "speeds": randn(g, (B, 1) if shared else (B, E, 1)), "tgt": torch.rand(B, generator=g).to(F32).to(F64), "c": LOSS_C}
    if kind == "lattice":
        d.update(speeds=lat(g, tuple(d["speeds"].shape), 8, 4), tgt=lat(g, (B,), 4, 4).abs(), c=(0.0, 0.5))
    return d


def loss_kinds(case):
    E, B, shared = case
    return KINDS if pow2(B if shared else B * E * E) else ("continuous",)


# ---------------------------------------------------------------------------------------------------------------------------------
# stem fold, bias pack

def eca_stem_fold(Gr, gate, w, ipe, cout, cin, taps, mut=""):
    """eca_stem_fold_dw_kernel, _ds_kernel: Gr [N, taps, coutp, cinp], gate [N, gate_ld], w [E, cout, cin, taps]
      dw[e, k, c, t] = sum over the expert's images of gate[n, c] * Gr[n, t, k, c]
      ds[n, c] = sum_{k, t} w[n // ipe, k, c, t] * Gr[n, t, k, c] for c < cin, zero in columns cin..gate_ld-1"""
    N, gld = gate.shape
    E = N // ipe
    g4 = Gr[:, :, :cout, :cin].permute(0, 2, 3, 1)                     # [N, cout, cin, taps]
    if mut == "tap":
        g4 = g4.flip(-1)
    terms = gate[:, None, :cin, None] * g4
    n = torch.arange(N)
    we = w[(n % E) if mut == "share" else n // ipe]
    t2 = we * g4
    ds, ds_abs = torch.zeros(N, gld, dtype=Gr.dtype), torch.zeros(N, gld, dtype=Gr.dtype)
    ds[:, :cin], ds_abs[:, :cin] = t2.sum((1, 3)), t2.abs().sum((1, 3))
    if mut == "part":
        terms = terms.clone()
        terms[ipe - 1::ipe] = 0
    return {"dw": terms.reshape(E, ipe, cout, cin, taps).sum(1), "dw_abs": terms.abs().reshape(E, ipe, cout, cin, taps).sum(1),
            "ds": ds, "ds_abs": ds_abs}


def stem_fold_chains(ipe, cout, taps, gld):
    """dw: ipe terms in order.  ds: 256 // gld lanes per channel, each adds every lanes-th of the cout * taps terms, then one thread
    per channel adds the lanes (gld = 144: one lane per channel, 112 idle threads)"""
    lanes = 256 // gld
    return ipe, cdiv(cout * taps, lanes) + lanes


# (E, ipe, cout, coutp, cin, gate_ld, cinp, ks)
STEM_FOLD_CASES = [(2, 3, 5, 64, cin, gld, cinp, ks) for cin, gld, cinp in ((12, 16, 16), (138, 144, 144)) for ks in (1, 3)]


@functools.lru_cache(maxsize=None)
def stem_fold_data(case, kind):
    """the pad region of Gr (k >= cout, c >= cin) and of gate (c >= cin) is NaN: neither kernel may read it.  lattice: multiples of
    1/4 up to 2 (products of 1/16, sums of at most 45 of them)"""
    E, ipe, cout, coutp, cin, gld, cinp, ks = case
    g = gen("stem_fold", case, kind)
    N, taps = E * ipe, ks * ks
    mk = (lambda s: lat(g, s, 8, 4)) if kind == "lattice" else (lambda s: randn(g, s))
    Gr, gate = torch.full((N, taps, coutp, cinp), float("nan"), dtype=F64), torch.full((N, gld), float("nan"), dtype=F64)
    Gr[:, :, :cout, :cin], gate[:, :cin] = mk((N, taps, cout, cin)), mk((N, cin))
    return {"G": Gr, "gate": gate, "w": mk((E, cout, cin, taps))}


def pack_bias(src, coutp):
    """src [E, cout] -> [E, coutp], zero pad"""
    out = torch.zeros(src.shape[0], coutp, dtype=src.dtype)
    out[:, :src.shape[1]] = src
    return {"dst": out}


PACK_BIAS_CASES = [(3, 5, 64), (3, 300, 320), (1, 64, 64)]          # (E, cout, coutp); 320: two workgroups per expert
