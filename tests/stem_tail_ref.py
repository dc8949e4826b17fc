"""Float64 reference of every entry point of csrc/stem_tail.hip, and the two input generators of its tests.

Pure torch on the CPU.  Each function takes exactly the tensors its kernel takes (activations NHWC ``[N, H, W, C]`` with image n
owned by expert ``n // ipe``, constants ``[E, C]``), upcast to float64, and returns a dict.  The twelve constants are independent
inputs (``CONSTS`` gives the order of struct TailConsts); nothing here assumes they are the batch statistics of the data.

    a2 = relu((z - mu2)*sc2 + sh2)      a3 = relu((a2 - mu1)*sc1 + sh1)      y = maxpool3x3/s2/p1(a3 rounded to the storage type)
    xhat1 = (a2 - mu1)*is1              da2 = g3*sc1 + xhat1*P + Q           P = -sc1*c21, Q = -sc1*c11
    xhat2 = (z - mu2)*is2               dz2 = g2*sc2 + xhat2*R + S           R = -sc2*c22, S = -sc2*c12

Every sum comes with ``abs_*``: the sum of the absolute values of its terms; ``dz2`` comes with ``dz2_abs``, the sum of the
absolute values of its addends with every difference expanded (|z| + |mu2| for z - mu2, ...).  The float32 error bounds of
tests/test_stem_tail_gpu.py are multiples of these.
"""
import functools
import math

import torch

CONSTS = ("sc2", "sh2", "sc1", "sh1", "mu1", "is1", "mu2", "is2", "c11", "c21", "c12", "c22")
F64 = torch.float64


def up(t):
    return t.detach().cpu().to(F64)


def round_to(x, dtype):
    """float64 -> the value the kernel stores: float32 arithmetic result, rounded to nearest-even to ``dtype``"""
    if dtype == F64:
        return x
    return x.to(torch.float32).to(dtype).to(F64)


def bc(c, ipe):
    """[E, C] -> [N, 1, 1, C]"""
    return c.repeat_interleave(ipe, 0)[:, None, None, :]


def esum(t, E):
    """[N, ..., C] -> [E, C]"""
    return t.reshape(E, -1, t.shape[-1]).sum(1)


def out_size(h):
    return (h - 1) // 2 + 1


def chain(z, k, ipe):
    """the re-derived activations: u = z - mu2, a2, p3 (a3 before its ReLU), and magnitudes of their addends"""
    u = z - bc(k["mu2"], ipe)
    p2 = u * bc(k["sc2"], ipe) + bc(k["sh2"], ipe)
    a2 = p2.clamp_min(0)
    out = {"u": u, "p2": p2, "a2": a2,
           "p2_mag": (u * bc(k["sc2"], ipe)).abs() + bc(k["sh2"], ipe).abs()}
    if "sc1" in k:
        d1 = a2 - bc(k["mu1"], ipe)
        out["d1"] = d1
        out["p3"] = d1 * bc(k["sc1"], ipe) + bc(k["sh1"], ipe)
        out["p3_mag"] = (d1 * bc(k["sc1"], ipe)).abs() + bc(k["sh1"], ipe).abs()
        # every addend of p3 down to z: what a float32 evaluation's error is proportional to
        out["p3_full"] = (out["p2_mag"] + bc(k["mu1"], ipe).abs()) * bc(k["sc1"], ipe).abs() + bc(k["sh1"], ipe).abs()
    return out


def stats(z, sc2, sh2, mu2, ipe):
    E = sc2.shape[0]
    ch = chain(z, {"sc2": sc2, "sh2": sh2, "mu2": mu2}, ipe)
    a2, u = ch["a2"], ch["u"]
    zi = z.reshape(E, -1, z.shape[-1])[:, 0]                              # the expert's first pixel
    shiftc = ((zi - mu2) * sc2 + sh2).clamp_min(0)
    d = a2 - bc(shiftc, ipe)
    m = (a2 > 0).to(z.dtype)
    terms = {"s1": d, "s2": d * d, "x0": m, "x1": m * u, "x2": a2 * u}
    out = {"shiftc": shiftc, "terms": terms, "chain": ch}
    for n, t in terms.items():
        out[n], out["abs_" + n] = esum(t, E), esum(t.abs(), E)
    return out


def windows(t, fill):
    """[N, H, W, C] -> [9, N, Ho, Wo, C]: tap 3*r + q of every 3x3/s2/p1 window, ``fill`` outside the image"""
    n, h, w, c = t.shape
    ho, wo = out_size(h), out_size(w)
    pad = torch.full((n, 2 * ho + 2, 2 * wo + 2, c), fill, dtype=t.dtype)
    pad[:, 1:h + 1, 1:w + 1] = t
    return torch.stack([pad[:, r:r + 2 * ho:2, q:q + 2 * wo:2] for r in range(3) for q in range(3)])


def pool(z, sc2, sh2, sc1, sh1, mu2, mu1, ipe, dtype):
    ch = chain(z, {"sc2": sc2, "sh2": sh2, "mu2": mu2, "sc1": sc1, "sh1": sh1, "mu1": mu1}, ipe)
    a3 = round_to(ch["p3"].clamp_min(0), dtype)
    cand = windows(a3, -math.inf)
    y = cand.max(0).values
    idx = torch.arange(9).view(9, 1, 1, 1, 1).expand_as(cand)
    tap = torch.where(cand == y, idx, torch.full_like(idx, 9)).min(0).values        # FIRST maximum in (row, column) scan order
    a2w = windows(ch["a2"], 0.0).gather(0, tap[None])[0]
    code = (tap | torch.where(a2w > 0, 0x80, 0)).to(torch.uint8)
    return {"y": y, "code": code, "tap": tap, "cand": cand, "a3": a3, "chain": ch}


def scatter_taps(dpool, amax, h, w):
    """the pooled gradient sent back to the winning taps of ``amax`` (bit 7 ignored; a tap outside the image receives nothing)"""
    n, ho, wo, c = dpool.shape
    pad = torch.zeros(n, 2 * ho + 2, 2 * wo + 2, c, dtype=dpool.dtype)
    tap = (amax & 0x7f).to(torch.int64)
    for r in range(3):
        for q in range(3):
            pad[:, r:r + 2 * ho:2, q:q + 2 * wo:2] += dpool * (tap == 3 * r + q)
    return pad[:, 1:h + 1, 1:w + 1].clone()


def bwd(phase, z, dpool, amax, k, ipe):
    """phase 1: sums of g3, g3*xhat1; phase 2: sums of g2, g2*xhat2; phase 3: dz2.  ``k``: dict of the constants by name"""
    E = k["sc2"].shape[0]
    n, h, w, c = z.shape
    b = lambda name: bc(k[name], ipe)
    ch = chain(z, k, ipe)
    a2, u = ch["a2"], ch["u"]
    zero = torch.zeros((), dtype=z.dtype)
    g3 = torch.where(ch["p3"] > 0, scatter_taps(dpool, amax, h, w), zero)
    xhat1 = ch["d1"] * b("is1")
    out = {"chain": ch, "g3": g3, "xhat1": xhat1}
    if phase == 1:
        terms = {"s1": g3, "s2": g3 * xhat1}
    else:
        P, Q = -b("sc1") * b("c21"), -b("sc1") * b("c11")
        m2 = (a2 > 0).to(z.dtype)
        g2 = torch.where(a2 > 0, g3 * b("sc1") + (xhat1 * P + Q), zero)
        xhat2 = u * b("is2")
        out.update(g2=g2, xhat2=xhat2, xhat1P=xhat1 * P)
        if phase == 2:
            terms = {"s1": g2, "s2": g2 * xhat2}
        else:
            R, S = -b("sc2") * b("c22"), -b("sc2") * b("c12")
            out["xhat2R"] = xhat2 * R
            out["dz2"] = g2 * b("sc2") + (xhat2 * R + S)
            a2_mag = (z.abs() + b("mu2").abs()) * b("sc2").abs() + b("sh2").abs()
            g3_mag = scatter_taps(dpool.abs(), amax, h, w) * (ch["p3"] > 0)          # a pixel can win up to four windows
            g2_mag = m2 * ((g3_mag * b("sc1")).abs() + (a2_mag + b("mu1").abs()) * (b("is1") * P).abs() + Q.abs())
            out["dz2_abs"] = g2_mag * b("sc2").abs() + (z.abs() + b("mu2").abs()) * (b("is2") * R).abs() + S.abs()
            return out
    out["terms"] = terms
    for nme, t in terms.items():
        out[nme], out["abs_" + nme] = esum(t, E), esum(t.abs(), E)
    return out


def pooled(y, dpool, amax, k, E):
    """sums over the pooled tensors: g, g*xhat1, g*m, g*m*xhat2 with xhat1, xhat2 recovered from y (sc == 0: contributes 0)"""
    ipe = y.shape[0] // E
    b = lambda t: bc(t, ipe)
    inv = lambda t: torch.where(t != 0, 1.0 / torch.where(t != 0, t, torch.ones_like(t)), torch.zeros_like(t))
    g = dpool * (y > 0)
    da = (y - b(k["sh1"])) * b(inv(k["sc1"]))
    gm = g * ((amax & 0x80) != 0)
    u = (da + b(k["mu1"]) - b(k["sh2"])) * b(inv(k["sc2"]))
    terms = [g, g * (da * b(k["is1"])), gm, gm * (u * b(k["is2"]))]
    return {"terms": terms, "da": da, "u": u,
            "sums": torch.stack([esum(t, E) for t in terms], 1), "abs": torch.stack([esum(t.abs(), E) for t in terms], 1)}


def combine(part4, part_x, k, count):
    """part4 [E, np4, 4, C], part_x [E, npx, 3, C] -> out1, out2 [E, 2, C] and the sums of the absolute values of their addends"""
    p, x = part4.sum(1), part_x.sum(1)
    pa, xa = part4.abs().sum(1), part_x.abs().sum(1)
    sc1, mu1, is1, is2 = k["sc1"], k["mu1"], k["is1"], k["is2"]
    P, Q = -sc1 * (p[:, 1] / count), -sc1 * (p[:, 0] / count)
    Pa, Qa = sc1.abs() * (pa[:, 1] / count), sc1.abs() * (pa[:, 0] / count)
    M0, Mu, Au = x[:, 0], x[:, 1], x[:, 2]
    Mx1, Mx2, Mx12 = is1 * mu1 * (count - M0), is2 * Mu, is1 * is2 * (Au - mu1 * Mu)
    Mx1a, Mx2a, Mx12a = (is1 * mu1).abs() * (count + xa[:, 0]), is2.abs() * xa[:, 1], (is1 * is2).abs() * (xa[:, 2] + mu1.abs() * xa[:, 1])
    out2 = torch.stack([sc1 * p[:, 2] + P * Mx1 + Q * M0, sc1 * p[:, 3] + P * Mx12 + Q * Mx2], 1)
    abs2 = torch.stack([sc1.abs() * pa[:, 2] + Pa * Mx1a + Qa * xa[:, 0], sc1.abs() * pa[:, 3] + Pa * Mx12a + Qa * Mx2a], 1)
    return {"out1": p[:, :2].clone(), "abs1": pa[:, :2].clone(), "out2": out2, "abs2": abs2}


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_stem_tail_gpu.py (checked on the CPU by tests/test_stem_tail_cpu.py for what the GPU tests assume)

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(2, 2, 37, 21), (1, 3, 16, 8), (3, 1, 1, 1), (1, 2, 2, 3), (2, 1, 33, 7), (1, 2, 18, 50)]
# (E, B, H, W, C, dtype)
CASES = [s + (64, d) for s in SHAPES for d in (BF16, F32)] + [SHAPES[0] + (32, BF16), SHAPES[0] + (128, BF16)]
ZERO_SC1_CHANNEL = 3                  # lattice cases: sc1 == 0 there (a3 constant: every window an all-way tie)
LATTICE_G = 10                        # every lattice intermediate is a multiple of 2^-10


def case_id(case):
    e, b, h, w, c, d = case
    return f"{e}x{b}x{h}x{w}-C{c}-{'bf16' if d == BF16 else 'f32'}"


def _seed(case):
    e, b, h, w, c, d = case
    return 1000 * h + 10 * w + e + b + c + (0 if d == BF16 else 5)


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    """z2, dpool, shifts, means and the c constants: multiples of 1/4 in [-3/2, 3/2] / [-1/2, 1/2]; gammas and inverse standard
    deviations from {-1, 1/2, 1, 2}.  Coarse on purpose: exact ties, zero plateaus after each ReLU and a2 == 0 are everywhere."""
    E, B, H, W, C, dtype = case
    g = torch.Generator().manual_seed(_seed(case))
    N, Ho, Wo = E * B, out_size(H), out_size(W)
    q = lambda shape, lim: torch.randint(-lim, lim + 1, shape, generator=g).to(F64) / 4
    pick = lambda: torch.tensor([-1.0, 0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (E, C), generator=g)]
    z, dpool = q((N, H, W, C), 6), q((N, Ho, Wo, C), 6)
    k = {}
    for name in CONSTS:
        k[name] = pick() if name in ("sc2", "sc1", "is1", "is2") else q((E, C), 2)
    k["sc1"][:, ZERO_SC1_CHANNEL] = 0.0
    k["sh1"][:, ZERO_SC1_CHANNEL] = 0.5           # the constant a3 is positive: the gradient reaches the first valid tap
    return {"z": z, "dpool": dpool, "k": k}


def bf16_boundary_distance(v):
    """distance of v >= 0 to the nearest rounding boundary of bfloat16 (the midpoint of two neighbouring bfloat16 values)"""
    _, ex = torch.frexp(v.clamp_min(1e-300))                     # v = m * 2^ex, m in [1/2, 1)
    ulp = torch.ldexp(torch.ones_like(v), ex - 8)
    frac = torch.remainder(v / ulp, 1.0)
    return (frac - 0.5).abs() * ulp


def relu_ambiguous(ch, tol=2.0 ** -18):
    """the issue's rule: a ReLU pre-activation (of a2 or of a3) within tol * (|x*sc| + |sh|) of zero"""
    return (ch["p2"].abs() <= tol * ch["p2_mag"]) | (ch["p3"].abs() <= tol * ch["p3_mag"])


def round_ambiguous(ch, dtype, tol=2.0 ** -18):
    """the issue's rule: a3 within relative tol of a rounding boundary of the storage type.  float32 storage rounds nothing (the
    kernel keeps its float32 a3 as it is), so it has no such boundary; its near-ties are found by ``near_tie``."""
    a3 = ch["p3"].clamp_min(0)
    if dtype != BF16:
        return torch.zeros_like(a3, dtype=torch.bool)
    return (a3 > 0) & (bf16_boundary_distance(a3) <= tol * a3)


def _generator_ambiguous(ch, dtype, tol=2.0 ** -18):
    """what continuous_case() redraws: both rules above with the margin taken from EVERY addend down to z (never smaller than the
    rules' own), so that the float32 kernel provably lands on the reference's side of each ReLU and each rounding boundary"""
    a3 = ch["p3"].clamp_min(0)
    amb = (ch["p2"].abs() <= tol * ch["p2_mag"]) | (ch["p3"].abs() <= tol * ch["p3_full"])
    if dtype == BF16:
        amb |= (a3 > 0) & (bf16_boundary_distance(a3) <= tol * ch["p3_full"])
    return amb


@functools.lru_cache(maxsize=None)
def continuous_case(case):
    """randn activations in the storage type with ordinary BatchNorm-like constants; elements that would be ambiguous are redrawn"""
    E, B, H, W, C, dtype = case
    g = torch.Generator().manual_seed(_seed(case) + 1)
    N, Ho, Wo = E * B, out_size(H), out_size(W)
    rnd = lambda shape: torch.randn(shape, generator=g).to(dtype).to(F64)
    u = lambda lo, hi: (torch.rand(E, C, generator=g) * (hi - lo) + lo).to(torch.float32).to(F64)
    z, dpool = rnd((N, H, W, C)), rnd((N, Ho, Wo, C))
    rng = {"sc2": (.5, 1.5), "sh2": (-.3, .3), "sc1": (.5, 1.5), "sh1": (-.3, .3), "mu1": (.2, .5), "is1": (.8, 1.2),
           "mu2": (-.1, .1), "is2": (.8, 1.2), "c11": (-.01, .01), "c21": (-.01, .01), "c12": (-.01, .01), "c22": (-.01, .01)}
    k = {name: u(*rng[name]) for name in CONSTS}
    for _ in range(64):
        for _ in range(64):
            amb = _generator_ambiguous(chain(z, k, B), dtype)
            if not amb.any():
                break
            z = torch.where(amb, rnd(z.shape), z)
        else:
            raise AssertionError("continuous_case: ambiguous elements left after 64 redraws")
        # ... and the (expert, channel) accumulators whose TERMS no float32 evaluation can deliver to a few roundings of |term|
        # (a term through a cancelling difference such as a2 - mu1, alone or nearly alone in its sum: 1x1 and 2x3 images)
        bad = bc(term_error_share(case, z, dpool, k) > TERM_ERROR_BUDGET, B)
        if not bad.any():
            break
        z, dpool = torch.where(bad, rnd(z.shape), z), torch.where(bad, rnd(dpool.shape), dpool)
    else:
        raise AssertionError("continuous_case: ill-conditioned accumulators left after 64 redraws")
    return {"z": z, "dpool": dpool, "k": k}


TERM_ERROR_BUDGET = 6.0      # of the 8 roundings the bound (L + 8) 2^-24 sum|term| grants the terms; L is the additions' share


def term_error_share(case, z, dpool, k):
    """[E, C]: over every sum of every reduction kernel, sum|term_f32 - term| / (2^-24 sum|term|), the terms evaluated by these
    same reference formulas in float32 on the CPU (plain, unfused).  This measures the DATA, not a kernel: the bound of the GPU
    test presumes that a float32 evaluation delivers each sum's terms to within 8 * 2^-24 of their absolute sum, which holds for
    sums of many terms and cannot hold for a sum of one term that went through a cancelling difference."""
    E, B, H, W, C, dtype = case
    po = pool(z, k["sc2"], k["sh2"], k["sc1"], k["sh1"], k["mu2"], k["mu1"], B, dtype)
    f = lambda t: t.to(torch.float32)
    k32 = {n: f(t) for n, t in k.items()}
    pairs = []
    a, b = stats(z, k["sc2"], k["sh2"], k["mu2"], B), stats(f(z), k32["sc2"], k32["sh2"], k32["mu2"], B)
    pairs += [(a["terms"][n], b["terms"][n]) for n in a["terms"]]
    for ph in (1, 2):
        a, b = bwd(ph, z, dpool, po["code"], k, B), bwd(ph, f(z), f(dpool), po["code"], k32, B)
        pairs += [(a["terms"][n], b["terms"][n]) for n in a["terms"]]
    a, b = pooled(po["y"], dpool, po["code"], k, E), pooled(f(po["y"]), f(dpool), po["code"], k32, E)
    pairs += list(zip(a["terms"], b["terms"]))
    share = torch.zeros(E, C, dtype=F64)
    for t64, t32 in pairs:
        err, mag = esum((t32.to(F64) - t64).abs(), E), esum(t64.abs(), E)
        share = torch.maximum(share, torch.where(err > 0, err / (2.0 ** -24 * mag).clamp_min(1e-300), torch.zeros_like(err)))
    return share


def near_tie(po, full_w, tol=2.0 ** -18):
    """outputs whose arg-max a float32 evaluation may resolve differently: a candidate other than the winner, of positive value,
    within tol * (sum of the absolute addends) of the maximum.  (Equal zeros are exact in both and stay first-wins.)"""
    idx = torch.arange(9).view(9, 1, 1, 1, 1)
    other = idx != po["tap"][None]
    return (other & (po["cand"] > 0) & (po["cand"] >= po["y"][None] - tol * full_w)).any(0)


def ambiguous_outputs(case, data):
    """per pooled output: is any candidate of its window ambiguous (ReLU or rounding rule), or the maximum a near-tie"""
    E, B, H, W, C, dtype = case
    k = data["k"]
    po = pool(data["z"], k["sc2"], k["sh2"], k["sc1"], k["sh1"], k["mu2"], k["mu1"], B, dtype)
    ch = po["chain"]
    elem = relu_ambiguous(ch) | round_ambiguous(ch, dtype)
    amb = windows(elem.to(F64), 0.0).sum(0) > 0
    if dtype != BF16:
        amb |= near_tie(po, windows(ch["p3_full"], 0.0))
    return {"outputs": amb, "elements": elem, "pool": po}
