"""Reference of every stand-alone BatchNorm pass of csrc/elementwise.hip, one function per entry point, and the input generators
of its tests (tests/test_bn_cpu.py, tests/test_bn_gpu.py).

Pure torch on the CPU.  Each function takes what its kernel takes and computes in the dtype it is handed: float64 is the
reference, float32 is the plain CPU evaluation that tests/test_bn_cpu.py holds against the bounds of the GPU tests.  Activations
are rows ``[E * rpe, C]`` (any leading shape whose product is E * rpe), expert e owning rows [e * rpe, (e + 1) * rpe); per-channel
constants are ``[E, C]``.  A partitioned sum comes with ``abs``: the sum of the absolute values of the same terms, partition by
partition; a stored tensor comes with ``mag``: the sum of the absolute values of its addends with every difference expanded
(|x| + |mean| for x - mean).  The float32 error bounds of tests/test_bn_gpu.py are multiples of these.

Out of scope: the fp8 side output of bn_apply; the ECA kernels are in tests/eca_head_ref.py.  The convolution-fused forms (statistics epilogue, BatchNorm on
load, PMOE_RES_DBN, the bn_fused weight gradient) are in tests/conv_ref.py, built on bn_apply / bn_bwd_apply of this file.
"""
import functools

import torch

from tests.stem_tail_ref import BF16, F32, F64, bf16_boundary_distance, round_to

EPS24 = 2.0 ** -24


def ve(dtype):
    """elements of a 16-byte vector"""
    return 8 if dtype == BF16 else 4


def cdiv(a, b):
    return -(-a // b)


def rows(t, E):
    """[..., C] -> [E, rpe, C]"""
    return t.reshape(E, -1, t.shape[-1])


def partition(terms, nparts):
    """[G, R, W] -> sums and sums of absolute values [G, nparts, W] over partitions of rpp = ceil(R / nparts) consecutive rows:
    partition p owns rows [p * rpp, min((p + 1) * rpp, R)); a partition past the end is empty and gives zeros"""
    G, R, W = terms.shape
    rpp = cdiv(R, nparts)
    pad = torch.zeros(G, rpp * nparts - R, W, dtype=terms.dtype)
    t = torch.cat([terms, pad], 1).reshape(G, nparts, rpp, W)
    return t.sum(2), t.abs().sum(2)


def colstats(x, rpe, E, C, ld, coff, nparts, use_shiftc=True):
    """colstats_kernel<T, 0>: x [E * rpe, ld], the channel window [coff, coff + C) of it (ld <= 0: dense).
    part[e, p, 0] = sum (x - c), part[e, p, 1] = sum (x - c)^2 over partition p, c = row 0 of expert e, also written to shiftc
    (no shiftc: c = 0)."""
    if ld <= 0:
        ld, coff = C, 0
    xw = x.reshape(E, rpe, ld)[:, :, coff:coff + C]
    c = xw[:, 0].clone() if use_shiftc else torch.zeros(E, C, dtype=x.dtype)
    d = xw - c[:, None]
    (s1, a1), (s2, a2) = partition(d, nparts), partition(d * d, nparts)
    return {"part": torch.stack([s1, s2], 2), "abs": torch.stack([a1, a2], 2), "shiftc": c}


def relu_mask(relu, y, x, mean, scale, shift, E):
    """the three mask forms of the backward kernels: none (relu off), from the saved output y > 0, or -- y None -- recomputed
    as (x - mean) * scale + shift > 0"""
    xr = rows(x, E)
    if not relu:
        return torch.ones_like(xr, dtype=torch.bool)
    if y is not None:
        return rows(y, E) > 0
    return (xr - mean[:, None]) * scale[:, None] + shift[:, None] > 0


def bn_bwd_reduce(dy, y, x, mean, invstd, scale, shift, E, relu, nparts):
    """colstats_kernel<T, 1>: g = dy where the mask holds, else 0; part[e, p, 0] = sum g, part[e, p, 1] = sum g * (x - mean) *
    invstd; gmask = g."""
    m = relu_mask(relu, y, x, mean, scale, shift, E)
    g = torch.where(m, rows(dy, E), torch.zeros((), dtype=dy.dtype))
    t2 = g * (rows(x, E) - mean[:, None]) * invstd[:, None]
    (s1, a1), (s2, a2) = partition(g, nparts), partition(t2, nparts)
    return {"part": torch.stack([s1, s2], 2), "abs": torch.stack([a1, a2], 2), "gmask": g.reshape(dy.shape)}


def reduce_partials(part_in, nout):
    """reduce_partials_kernel: [E, nin, width] -> [E, nout, width], output o sums per = ceil(nin / nout) consecutive input rows;
    outputs past the end are zero"""
    s, a = partition(part_in, nout)
    return {"out": s, "abs": a}


def bn_finalize(part, count, gamma, beta, running, momentum, eps, training, shiftc):
    """bn_finalize_kernel.  part [E, nparts, 2, C]; gamma, beta, shiftc: [E, C] or None; running: None or (rmean [E, C],
    rvar [E, C], on [E] bool) -- an expert whose table entry is null gets no update.
    training: md = sum part[:, :, 0] / count, var = max(sum part[:, :, 1] / count - md^2, 0), mean = md + shiftc;
              running = (1 - momentum) * running + momentum * (mean | var * count / (count - 1), var itself if count == 1)
    eval:     mean, var = running
    invstd = 1 / sqrt(var + eps), scale = gamma * invstd (gamma null: 1), shift = beta (null: 0)."""
    E, _, _, C = part.shape
    dt = part.dtype
    out = {}
    if training:
        t1, t2 = part[:, :, 0].sum(1), part[:, :, 1].sum(1)
        out["abs1"], out["abs2"] = part[:, :, 0].abs().sum(1), part[:, :, 1].abs().sum(1)
        md = t1 / count
        var = (t2 / count - md * md).clamp_min(0)
        mean = md + shiftc if shiftc is not None else md
        out["md"] = md
        if running is not None:
            rm, rv, on = running
            unb = var * count / (count - 1) if count > 1 else var
            on = on[:, None]
            out["unb"] = unb
            out["rmean"] = torch.where(on, (1 - momentum) * rm + momentum * mean, rm)
            out["rvar"] = torch.where(on, (1 - momentum) * rv + momentum * unb, rv)
    else:
        mean, var = running[0].clone(), running[1].clone()
    invstd = 1 / torch.sqrt(var + eps)
    out.update(mean=mean, var=var, invstd=invstd,
               scale=invstd * gamma if gamma is not None else invstd.clone(),
               shift=beta.clone() if beta is not None else torch.zeros(E, C, dtype=dt))
    return out


def bn_bwd_finalize(part, count):
    """bn_bwd_finalize_kernel: dbeta = sum part[:, :, 0], dgamma = sum part[:, :, 1], c1 = dbeta / count, c2 = dgamma / count"""
    t1, t2 = part[:, :, 0].sum(1), part[:, :, 1].sum(1)
    return {"dbeta": t1, "dgamma": t2, "c1": t1 / count, "c2": t2 / count,
            "abs1": part[:, :, 0].abs().sum(1), "abs2": part[:, :, 1].abs().sum(1)}


def bn_apply(x, res, scale, shift, mean, E, relu, dtype):
    """bn_apply_kernel: y = [relu]((x - mean) * scale + shift [+ res]), rounded to the storage type.  ``pre``: before the ReLU
    and the rounding.  (Where y lands -- dense or a channel window -- is the caller's business.)"""
    xr = rows(x, E)
    pre = (xr - mean[:, None]) * scale[:, None] + shift[:, None]
    mag = (xr.abs() + mean.abs()[:, None]) * scale.abs()[:, None] + shift.abs()[:, None]
    if res is not None:
        pre, mag = pre + rows(res, E), mag + rows(res, E).abs()
    y = pre.clamp_min(0) if relu else pre
    return {"y": round_to(y, dtype).reshape(x.shape), "pre": pre.reshape(x.shape), "mag": mag.reshape(x.shape)}


def pool2(y):
    """[N, H, W, C] -> MaxPool2d(2, 2)"""
    n, h, w, c = y.shape
    return y.reshape(n, h // 2, 2, w // 2, 2, c).amax((2, 4))


def bn_apply_pool2(x, scale, shift, mean, E, relu, dtype):
    """bn_apply_pool2_kernel: x [N, H, W, C]; y as bn_apply without residual, pooled = the 2x2 maximum of the STORED y"""
    out = bn_apply(x, None, scale, shift, mean, E, relu, dtype)
    out["pooled"] = pool2(out["y"])
    return out


def gap_sums(y, nparts):
    """[N, H, W, C] -> per-image partitioned sums over the HW pixels: (sums, sums of absolute values) [N, nparts, C]"""
    return partition(y.reshape(y.shape[0], -1, y.shape[-1]), nparts)


def bn_apply_gap(x, scale, shift, mean, nparts, ipe, relu, dtype):
    """bn_apply_gap_kernel: y as bn_apply without residual; part[n, p] = sum over partition p of image n's pixels of the STORED y"""
    out = bn_apply(x, None, scale, shift, mean, x.shape[0] // ipe, relu, dtype)
    out["part"], out["abs"] = gap_sums(out["y"], nparts)
    return out


def gap_partial(a, b, nparts, b_shared_ipe):
    """gap_partial_kernel: part[n, p] = sum of a (b None) or of a * b over partition p of image n's pixels; b_shared_ipe > 0:
    b holds b_shared_ipe images and image n reads b[n % b_shared_ipe]"""
    t = a
    if b is not None:
        idx = torch.arange(a.shape[0])
        t = a * b[idx % b_shared_ipe if b_shared_ipe > 0 else idx]
    s, ab = gap_sums(t, nparts)
    return {"part": s, "abs": ab}


def bn_bwd_apply(dy, y, x, mean, invstd, scale, shift, c1, c2, E, relu, dtype):
    """bn_bwd_apply_kernel: g = dy under the mask (relu_mask), dx = g * A + ((x - mean) * Bx + K) with A = scale,
    Bx = -scale * invstd * c2, K = -scale * c1; gm = g.  dx is rounded to the storage type; ``dx_raw`` is not."""
    m = relu_mask(relu, y, x, mean, scale, shift, E)
    g = torch.where(m, rows(dy, E), torch.zeros((), dtype=dy.dtype))
    xr = rows(x, E)
    A, Bx, K = scale[:, None], (-scale * invstd * c2)[:, None], (-scale * c1)[:, None]
    dx = g * A + ((xr - mean[:, None]) * Bx + K)
    mag = (g * A).abs() + (xr.abs() + mean.abs()[:, None]) * Bx.abs() + K.abs()
    return {"dx": round_to(dx, dtype).reshape(x.shape), "dx_raw": dx.reshape(x.shape), "mag": mag.reshape(x.shape),
            "gm": g.reshape(x.shape)}


# ---------------------------------------------------------------------------------------------------------------------------------
# chain lengths: the longest run of sequential float32 additions of one launch, read from the kernels

def stream_geometry(C, dtype):
    """colstats / gap kernels: CV channel vectors per row, RL = 256 // CV rows in flight per workgroup (CV that does not divide
    256 leaves 256 - RL * CV lanes idle)"""
    cv = C // ve(dtype)
    return cv, 256 // cv


def chain_stream(nrows, nparts, C, dtype):
    """colstats_kernel, gap_partial_kernel, bn_apply_gap_kernel: a thread adds every RL-th row of its partition of
    rpp = ceil(nrows / nparts) rows, then one thread per channel adds the RL lanes' sums from LDS"""
    _, RL = stream_geometry(C, dtype)
    return cdiv(cdiv(nrows, nparts), RL) + RL


def chain_reduce(nin, nout):
    """reduce_partials_kernel: one thread adds its output's per = ceil(nin / nout) rows in order"""
    return cdiv(nin, nout)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_bn_gpu.py; (E, ipe, H, W, C, dtype)

def _c(c_bf16, c_f32, dtype):
    return c_bf16 if dtype == BF16 else c_f32


DTYPES = (BF16, F32)
CASES = [s for d in DTYPES for s in (
    (1, 1, 1, 1, 64, d),                     # rpe = 1
    (3, 1, 7, 11, 64, d),                    # prime-ish rpe, three experts, ragged last partition
    (2, 2, 5, 3, _c(8, 4, d), d),            # CV = 1, RL = 256 > rpe
    (1, 1, 3, 5, _c(2048, 1024, d), d),      # CV = 256, RL = 1
    (2, 3, 9, 9, 128, d),
    (1, 2, 4, 4, 512, d))]
POOL_CASES = [(1, 1, 2, 2, 64, d) for d in DTYPES] + [(2, 3, 6, 2, 64, d) for d in DTYPES] + [(1, 2, 4, 10, 64, d) for d in DTYPES]
# gap_partial / bn_apply_gap: channel-vector counts 3 and 5 (idle lanes) and 8 / 16; HW = 1, 5, 77
GAP_CASES = [(2, 2, h, w, c, d) for d, cs in ((BF16, (24, 40, 64)), (F32, (12, 64))) for c in cs for h, w in ((1, 1), (1, 5), (7, 11))]
NPARTS = ("one", "four", "rows+1")
WINDOWS = ("3C+0", "3C+C", "3C+2C", "C+VE")


def nparts_of(name, nrows):
    return {"one": 1, "four": 4, "rows+1": nrows + 1}[name]


def window_of(name, C, dtype):
    """(ld, coff)"""
    return {"3C+0": (3 * C, 0), "3C+C": (3 * C, C), "3C+2C": (3 * C, 2 * C), "C+VE": (C + ve(dtype), ve(dtype))}[name]


def case_id(case):
    e, b, h, w, c, d = case
    return f"{e}x{b}x{h}x{w}-C{c}-{'bf16' if d == BF16 else 'f32'}"


def _seed(case):
    e, b, h, w, c, d = case
    return 100000 * e + 10000 * b + 1000 * h + 10 * w + c + (0 if d == BF16 else 5)


CONSTS = ("mean", "scale", "shift", "invstd", "c1", "c2")
ALL_EQUAL_CHANNEL, EXTREME_CHANNEL, FIRST_PLANTED_CHANNEL = 1, 2, 3
LATTICE_G = 4          # every lattice intermediate and stored value is a multiple of 2^-4 (every sum term too)


def planted(case):
    """[E, rpe, C] int: 0 = left alone; 1, 2, 3 = x puts the pre-activation (x - mean) * scale + shift at 0, one lattice step of
    x above, one below; 5, 6, 7 = the same for the residual form, by the residual"""
    E, B, H, W, C, _ = case
    r, c = torch.arange(B * H * W)[:, None], torch.arange(C)[None, :]
    code = (r + c) % 8 + 1
    code = torch.where((c >= FIRST_PLANTED_CHANNEL) & (code != 4) & (code != 8), code, torch.zeros_like(code))
    return code[None].expand(E, -1, -1)


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    """Data, residual, gradient, mean and c1: multiples of 1/4 (|x|, |res|, |dy| <= 2, the constants <= 1/2); shift: a multiple of
    1/2; scale in {-1, 1/2, 1, 2}, invstd in {1, 2}, c2 in {+-1/2, +-1}.  Then (x - mean) * scale + shift [+ res] is a multiple of
    1/8 below 8, dx a multiple of 1/16 below 16 (both hold in the 8 significant bits of bfloat16), every summed term a multiple of
    1/16 below 16, so that float32 arithmetic is exact in any order, fused or not.  Channel 1 is constant per expert (variance
    0), channel 2 has its maximum in row 0 (every deviation from row 0 is <= 0), and from channel 3 on three of every eight
    elements are planted on and next to the ReLU edge, three more by the residual (``planted``)."""
    E, B, H, W, C, dtype = case
    g = torch.Generator().manual_seed(_seed(case))
    rpe = B * H * W
    q = lambda shape, lim, den: torch.randint(-lim, lim + 1, shape, generator=g).to(F64) / den
    pick = lambda vals: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), (E, C), generator=g)]
    x, res, dy = q((E, rpe, C), 8, 4), q((E, rpe, C), 8, 4), q((E, rpe, C), 6, 4)
    k = {"mean": q((E, C), 2, 4), "shift": q((E, C), 1, 2), "c1": q((E, C), 2, 4), "scale": pick([-1.0, 0.5, 1.0, 2.0]),
         "invstd": pick([1.0, 2.0]), "c2": pick([-1.0, -0.5, 0.5, 1.0])}
    x[:, :, ALL_EQUAL_CHANNEL] = 0.75 - 0.5 * torch.arange(E, dtype=F64)[:, None]
    x[:, :, EXTREME_CHANNEL] = x[:, :, EXTREME_CHANNEL].clamp_max(1.75)
    x[:, 0, EXTREME_CHANNEL] = 2.0
    code = planted(case)
    step = torch.where((code & 3) == 2, 0.25, torch.where((code & 3) == 3, -0.25, 0.0)).to(F64)
    x0 = (k["mean"] - k["shift"] / k["scale"])[:, None] + step
    x = torch.where((code >= 1) & (code <= 3), x0, x)
    pre = (x - k["mean"][:, None]) * k["scale"][:, None] + k["shift"][:, None]
    res = torch.where(code >= 5, -pre + step / 2, res)
    shape = (E * B, H, W, C)
    return {"x": x.reshape(shape), "res": res.reshape(shape), "dy": dy.reshape(shape), "k": k}


def _bf16_ambiguous(v, margin, dtype):
    """v within ``margin`` of a rounding boundary of bfloat16 storage (float32 storage rounds nothing)"""
    if dtype != BF16:
        return torch.zeros_like(v, dtype=torch.bool)
    return (v != 0) & (bf16_boundary_distance(v.abs()) <= margin)


def forward_ambiguous(d, case, tol=2.0 ** -18):
    """elements where a float32 evaluation may land on the other side of a ReLU decision or of a storage rounding boundary:
    the pre-activation, without and with the residual, within tol * (sum of the absolute addends) of zero or of a boundary"""
    E, dtype, k = case[0], case[5], d["k"]
    amb = torch.zeros(d["x"].shape, dtype=torch.bool)
    for res in (None, d["res"]):
        a = bn_apply(d["x"], res, k["scale"], k["shift"], k["mean"], E, False, dtype)
        amb |= (a["pre"].abs() <= tol * a["mag"]) | _bf16_ambiguous(a["pre"], tol * a["mag"], dtype)
    return amb


def mask_forms(d, case):
    """the (relu, y) arguments of the backward kernels: no mask, the saved output of the residual form, the recomputed mask"""
    E, dtype, k = case[0], case[5], d["k"]
    y_res = bn_apply(d["x"], d["res"], k["scale"], k["shift"], k["mean"], E, True, dtype)["y"]
    return {"none": (False, None), "from_y": (True, y_res), "from_x": (True, None)}


def backward_ambiguous(d, case, tol=2.0 ** -18):
    """elements whose dx, under any of the three mask forms, lies within tol * (sum of the absolute addends) of a rounding
    boundary of the storage type"""
    E, dtype, k = case[0], case[5], d["k"]
    amb = torch.zeros(d["x"].shape, dtype=torch.bool)
    for relu, y in mask_forms(d, case).values():
        b = bn_bwd_apply(d["dy"], y, d["x"], k["mean"], k["invstd"], k["scale"], k["shift"], k["c1"], k["c2"], E, relu, dtype)
        amb |= _bf16_ambiguous(b["dx_raw"], tol * b["mag"], dtype)
    return amb


@functools.lru_cache(maxsize=None)
def continuous_case(case):
    """randn data in the storage type, scaled and offset per channel (channel 0: |mean| = 32 std), with BatchNorm-like
    constants; elements that would be ambiguous (forward_ambiguous, backward_ambiguous) are redrawn until none is left"""
    E, B, H, W, C, dtype = case
    g = torch.Generator().manual_seed(_seed(case) + 1)
    shape = (E * B, H, W, C)
    u = lambda lo, hi: (torch.rand(E, C, generator=g) * (hi - lo) + lo).to(F32).to(F64)
    std, off = (torch.rand(C, generator=g) + 0.5).to(F64), torch.randn(C, generator=g).to(F64)
    std[0], off[0] = 0.25, 8.0
    draw_x = lambda: (torch.randn(shape, generator=g).to(F64) * std + off).to(dtype).to(F64)
    draw = lambda: torch.randn(shape, generator=g).to(dtype).to(F64)
    k = {"mean": (off + u(-.1, .1) * std).to(F32).to(F64), "scale": u(.5, 1.5) / std * torch.where(u(0, 1) < 0.2, -1.0, 1.0),
         "shift": u(-.3, .3), "invstd": u(.8, 1.2) / std, "c1": u(-.1, .1), "c2": u(-.1, .1)}
    k = {n: t.to(F32).to(F64) for n, t in k.items()}
    d = {"x": draw_x(), "res": draw(), "dy": draw(), "k": k}
    for _ in range(64):
        # (a masked element's dx does not depend on dy: x is redrawn with it, so both rules are settled together)
        amb = forward_ambiguous(d, case) | backward_ambiguous(d, case)
        if not amb.any():
            break
        d["x"], d["res"], d["dy"] = torch.where(amb, draw_x(), d["x"]), torch.where(amb, draw(), d["res"]), torch.where(amb, draw(), d["dy"])
    else:
        raise AssertionError("continuous_case: ambiguous elements left after 64 redraws")
    return d


def case_data(case, kind):
    return lattice_case(case) if kind == "lattice" else continuous_case(case)


# ---------------------------------------------------------------------------------------------------------------------------------
# partial rows for reduce_partials and the finalize kernels (no upstream kernel)

FIN_NPARTS = (1, 31, 32, 33, 96, 97, 127, 128, 129, 1024, 2048)
FIN_C = (8, 32, 40, 64, 2048)
REDUCE_SHAPES = ((1, 1), (4, 2), (200, 128), (1024, 128), (129, 128))
LATTICE_EPS, LATTICE_MOMENTUM = 0.25, 0.125
LATTICE_VARS = (0.0, 0.75, 3.75, 15.75)                 # var + LATTICE_EPS: a power of 4
CONT_EPS = torch.tensor(1e-5, dtype=F32).item()         # the float32 values the launch receives
CONT_MOMENTUM = torch.tensor(0.1, dtype=F32).item()


def fin_configs(nparts, C):
    """(E, count, with shiftc, null tables) per (nparts, C): both expert counts, both counts, both shiftc forms and the null
    tables (gamma, beta and expert 1's running buffers) everywhere; three experts of the two largest products only once"""
    cfgs = [(1, 64, True, False), (3, 1, False, True), (3, 64, True, True), (1, 1, False, False)]
    if nparts * C > 2 ** 20:
        cfgs = [c for c in cfgs if c[0] == 1] + [(3, 64, True, True)] * (nparts * C <= 2 ** 21)
    return cfgs


def _distinct_rows(total, nparts, C):
    """[E, nparts, C] rows of distinct magnitude that sum to ``total`` [E, C]: +-(i + 1) * (1 + c % 3) / 4, the last row the
    balance"""
    i = torch.arange(nparts, dtype=F64)
    w = (torch.where(i % 2 == 0, 1.0, -1.0) * (i + 1))[None, :, None] * (1 + torch.arange(C) % 3).to(F64)[None, None, :] / 4
    w = w.expand(total.shape[0], -1, -1).clone()
    w[:, -1] = total - w[:, :-1].sum(1)
    return w


def finalize_lattice(E, nparts, C, count, seed):
    """partial rows that are multiples of 1/4, a power-of-two count, means that are multiples of 1/4 and variances from
    LATTICE_VARS: mean, var, var + eps, c1, c2 and the running mean are exact in float32; 1 / sqrt(var + eps) is 2, 1, 1/2 or 1/4.
    (count < 16: integer means, so that the sum of squares is still a multiple of 1/4.)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (E, C), generator=g).to(F64)
    md = ri(-6, 6) / 4 if count >= 16 else ri(-3, 3)
    var = torch.tensor(LATTICE_VARS, dtype=F64)[torch.randint(0, 4, (E, C), generator=g)]
    part = torch.stack([_distinct_rows(md * count, nparts, C), _distinct_rows((var + md * md) * count, nparts, C)], 2)
    return {"part": part, "var": var, "shiftc": ri(-8, 8) / 4, "rmean": ri(-8, 8) / 4,
            "rvar": torch.tensor(LATTICE_VARS[1:], dtype=F64)[torch.randint(0, 3, (E, C), generator=g)],
            "gamma": torch.tensor([-1.0, 0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (E, C), generator=g)],
            "beta": ri(-8, 8) / 4, "eps": LATTICE_EPS, "momentum": LATTICE_MOMENTUM}


def finalize_continuous(E, nparts, C, count, seed):
    """float32 randn rows, row i scaled by 1 + i / nparts (no two rows alike in magnitude); the first moments are scaled per
    channel so that the variance keeps at least 3/4 of the second moment (it is never near its clamp at 0)"""
    g = torch.Generator().manual_seed(seed)
    mag = (1 + torch.arange(nparts, dtype=F64) / nparts)[None, :, None]
    r1 = torch.randn(E, nparts, C, generator=g).to(F64) * mag
    r2 = (torch.randn(E, nparts, C, generator=g).to(F64).abs() + 0.1) * mag
    lim = 0.5 * torch.sqrt(r2.sum(1) / count)
    md = r1.sum(1) / count
    r1 = r1 * (lim / md.abs().clamp_min(1e-300)).clamp_max(1.0)[:, None]
    part = torch.stack([r1, r2], 2).to(F32).to(F64)
    u = lambda lo, hi: (torch.rand(E, C, generator=g) * (hi - lo) + lo).to(F32).to(F64)
    return {"part": part, "shiftc": u(-2, 2), "rmean": u(-1, 1), "rvar": u(.5, 1.5), "gamma": u(.5, 1.5), "beta": u(-.5, .5),
            "eps": CONT_EPS, "momentum": CONT_MOMENTUM}


def finalize_data(kind, E, nparts, C, count, seed):
    return (finalize_lattice if kind == "lattice" else finalize_continuous)(E, nparts, C, count, seed)


RSQRT_ULP = 2.0        # assumed error of HIP's rsqrtf in units in the last place (no documented figure at hand)


def finalize_bounds(ref, d, count, training, with_running):
    """Bounds of bn_finalize_kernel's outputs against ``ref`` (float64), from the kernel's arithmetic alone.

    The fold is in double: a sum of n <= 2048 float32 rows carries at most n 2^-53 sum|row| < 2^-40 sum|row|.  With
    S1 = sum|row1| / count, S2 = sum|row2| / count:
      mean    = float(md + shiftc):                              2^-24 |mean| + 2^-40 S1
      v       (double) = t2 / count - md^2:                      dv = 2^-40 (S2 + 2 |md| S1)   (+ a few 2^-53 v, inside the 2^-40)
      var     = float(v):                                        dv + 2^-24 var
      s       = float(var + eps):                                ds = dv + 2^-24 var + 2^-24 (var + eps)
      invstd  = rsqrtf(s), RSQRT_ULP units of <= 2^-23 relative: invstd * (ds / (2 (s - ds)) + RSQRT_ULP 2^-23)
                (|s'^-1/2 - s^-1/2| <= |s' - s| / (2 min(s, s')^3/2))
      scale   = float(gamma * invstd):                           one more rounding, 2^-24 relative
      running = float(float((1 - m) * old) + float(m * new)) with float(1 - m): four roundings of at most 2^-24 of the
                addends' absolute sum, plus m times the error of ``new`` (mean as above; the unbiased variance =
                float(v * count / (count - 1)): dv * count / (count - 1) + 2^-24 of itself)
    In eval mode dv = 0 and var is the running buffer itself (no rounding of var); the rest is the same."""
    var, eps, m = ref["var"], d["eps"], d["momentum"]
    out = {}
    if training:
        S1, S2 = ref["abs1"] / count, ref["abs2"] / count
        dmean = EPS24 * ref["mean"].abs() + 2.0 ** -40 * S1
        dv = 2.0 ** -40 * (S2 + 2 * ref["md"].abs() * S1)
        dvar = dv + EPS24 * var
    else:
        dmean = dv = dvar = torch.zeros_like(var)
    ds = dvar + EPS24 * (var + eps)
    rel = ds / (2 * (var + eps - ds)) + RSQRT_ULP * 2.0 ** -23
    out.update(mean=dmean, invstd=ref["invstd"] * rel, scale=ref["scale"].abs() * (rel + EPS24 + rel * EPS24),
               shift=torch.zeros_like(var))
    if training and with_running:
        f = count / (count - 1) if count > 1 else 1.0
        out["rmean"] = 4 * EPS24 * ((1 - m) * d["rmean"].abs() + m * ref["mean"].abs()) + m * dmean
        out["rvar"] = 4 * EPS24 * ((1 - m) * d["rvar"].abs() + m * ref["unb"].abs()) + m * (dv * f + EPS24 * ref["unb"])
    return out
