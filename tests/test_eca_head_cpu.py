"""What tests/test_eca_head_gpu.py assumes, proven without a GPU: the float64 reference (tests/eca_head_ref.py) agrees with torch's
own operators and autograd; lattice inputs keep a float32 evaluation bit-equal to float64 in more than one summation order;
continuous inputs stay clear of every rounding boundary and comparison; the reference in plain float32 stays within the bounds the
GPU test applies; the case tables reach every route, lane geometry and grid-stride loop that the launch code has; and a list of
deliberately wrong variants of the reference (mutants) breaks exact equality on the lattice and exceeds the bounds 16-fold on the
continuous kind."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import eca_head_ref as R

F64, F32, BF16 = R.F64, R.F32, R.BF16
EPS = R.EPS24


def c(t, dt):
    return None if t is None else t.to(dt)


def errof(got, ref):
    e = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs())
    return torch.nan_to_num(e, nan=float("inf"))


def flip_sum_axes(t, dims):
    return t.flip(dims) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------------------
# one runner per kernel: (case, kind, dt, mut, flip) -> {output: value as float64}; bounds(case, kind) -> {output: bound}, from the
# float64 reference; ``flip`` evaluates sums over reversed data (another summation order) where the kernel has a sum.
# A stored bfloat16 value and everything max pooling writes has bound 0: the GPU test demands equality there.

def zero_like(d):
    return {k: torch.zeros_like(v) for k, v in d.items()}


class Maxpool:
    cases = [(cs, k) for cs in R.MAXPOOL_CASES for k in R.KINDS]
    mutants = {"tap": None, "last": None}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        N, H, W, C, dtype = case
        d = R.maxpool_data(case, kind)
        f = R.maxpool_fwd(c(d["x"], dt), mut)
        own = R.maxpool_fwd(d["x"])["am"]
        return {"y": f["y"].to(F64), "am": f["am"].to(F64), "dx": R.maxpool_bwd(c(d["dy"], dt), own, H, W, dtype, mut)["dx"].to(F64),
                "dx_any": R.maxpool_bwd(c(d["dy"], dt), d["am_any"], H, W, dtype, mut)["dx"].to(F64)}

    @classmethod
    def bounds(cls, case, kind):
        return zero_like(cls.run(case, kind, F64))


class GapPartial:
    cases = [(cs, k) for cs in R.GAP_PARTIAL_CASES for k in R.KINDS]
    mutants = {"share": lambda cs: cs[7] == "ab_shared", "part": None}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, ipe, H, W, C, dtype, parts, form = case
        d = R.gap_partial_data(case, kind)
        a, b = c(d["a"], dt), c(d["b"], dt)
        nparts = R.nparts_of(parts, H * W)
        if flip and nparts == 1:
            a, b = a.flip((1, 2)), flip_sum_axes(b, (1, 2))
        return {"part": R.gap_partial(a, b, nparts, d["b_ipe"], mut)["part"].to(F64)}

    @staticmethod
    def bounds(case, kind):
        E, ipe, H, W, C, dtype, parts, form = case
        d = R.gap_partial_data(case, kind)
        nparts = R.nparts_of(parts, H * W)
        L = R.chain_stream(H * W, nparts, C, dtype)
        return {"part": (L + 8) * EPS * R.gap_partial(d["a"], d["b"], nparts, d["b_ipe"])["part_abs"]}


def stored_bounds(ref, dtype, key, extra=0.0, L=0):
    return {key: torch.zeros_like(ref[key]) if dtype == BF16 else R.stored_bound(ref[key], ref["mag"], extra, L)}


class GapFinish:
    cases = [(cs, k) for cs in R.GAP_FINISH_CASES for k in R.kinds_of(cs[3])]
    mutants = {"nohw": lambda cs: cs[3] > 1, "part": lambda cs: cs[2] > 1, "round2": lambda cs: cs[6] == F32}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        N, C, nparts, HW, ld, coff, dtype = case
        p = c(R.gap_finish_data(case, kind)["part"], dt)
        return {"out": R.gap_finish(p.flip(1) if flip else p, HW, dtype, mut)["out"]}

    @staticmethod
    def bounds(case, kind):
        N, C, nparts, HW, ld, coff, dtype = case
        return stored_bounds(R.gap_finish(R.gap_finish_data(case, kind)["part"], HW, dtype), dtype, "out", L=nparts)


class GapBwd:
    cases = [(cs, k) for cs in R.GAP_BWD_CASES for k in R.kinds_of(cs[1] * cs[2])]
    mutants = {"nohw": lambda cs: cs[1] * cs[2] > 1, "round2": lambda cs: cs[6] == F32}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        N, H, W, C, ld, coff, dtype = case
        return {"dx": R.gap_bwd(c(R.gap_bwd_data(case, kind)["g"], dt), H * W, C, coff, dtype, mut)["dx"][:, :1]}

    @staticmethod
    def bounds(case, kind):
        N, H, W, C, ld, coff, dtype = case
        r = R.gap_bwd(R.gap_bwd_data(case, kind)["g"], H * W, C, coff, dtype)
        return {"dx": (torch.zeros_like(r["raw"]) if dtype == BF16 else R.stored_bound(r["raw"], r["mag"]))[:, None]}


ECA = [(cs, k) for cs in R.ECA_CASES for k in R.kinds_of(cs[6])]


class EcaGate:
    cases = ECA
    mutants = {"tap": None, "share": lambda cs: cs[7], "creal": lambda cs: cs[3] < cs[2], "part": None, "nohw": lambda cs: cs[6] > 1}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, ipe, C, creal, k, nparts, HW, shared = case
        d = R.eca_data(case, kind)
        p = c(d["part"], dt)
        r = R.eca_gate(p.flip(1) if flip else p, HW, c(d["w"], dt), k, E * ipe, ipe, ipe if shared else 0, C, creal, mut)
        return {"gate": R.round_to(r["gate"].to(F64), F32), "gapmean": r["gapmean"].to(F64)}

    @staticmethod
    def bounds(case, kind):
        E, ipe, C, creal, k, nparts, HW, shared = case
        d = R.eca_data(case, kind)
        return R.eca_gate_bounds(R.eca_gate(d["part"], HW, d["w"], k, E * ipe, ipe, ipe if shared else 0, C, creal), nparts, k)


class EcaBwdSmall:
    cases = ECA
    mutants = {"tap": lambda cs: cs[4] > 1, "creal": lambda cs: cs[3] < cs[2], "part": None}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, ipe, C, creal, k, nparts, HW, shared = case
        d = R.eca_data(case, kind)
        p = c(d["dot_part"], dt)
        r = R.eca_bwd_small(p.flip(1) if flip else p, c(d["gate_in"], dt), c(d["gapmean_in"], dt), c(d["w_b"], dt), k, ipe, C, creal,
                            1.0 / HW, mut)
        return {"dgap": r["dgap"].to(F64), "dw": r["dw"].to(F64)}

    @staticmethod
    def bounds(case, kind):
        E, ipe, C, creal, k, nparts, HW, shared = case
        d = R.eca_data(case, kind)
        r = R.eca_bwd_small(d["dot_part"], d["gate_in"], d["gapmean_in"], d["w_b"], k, ipe, C, creal, 1.0 / HW)
        b = R.eca_bwd_small_bounds(r, nparts, k, ipe, C)
        return {"dgap": b["dgap"] + EPS * r["dgap"].abs(), "dw": b["dw"]}


class EcaScale:
    cases = [(cs, k) for cs in R.ECA_SCALE_CASES for k in R.KINDS]
    mutants = {"share": lambda cs: cs[5], "round2": lambda cs: cs[6] == F32}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, ipe, H, W, C, shared, dtype = case
        d = R.eca_scale_data(case, kind)
        return {"y": R.eca_scale(c(d["x"], dt), c(d["gate"], dt), ipe if shared else 0, dtype, mut)["y"]}

    @staticmethod
    def bounds(case, kind):
        E, ipe, H, W, C, shared, dtype = case
        d = R.eca_scale_data(case, kind)
        return stored_bounds(R.eca_scale(d["x"], d["gate"], ipe if shared else 0, dtype), dtype, "y")


class EcaApply:
    cases = [(cs, k) for cs in R.ECA_APPLY_CASES for k in R.kinds_of(cs[1] * cs[2])]
    mutants = {"nohw": None, "round2": lambda cs: cs[4] == F32}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        d = R.eca_apply_data(case, kind)
        return {"dx": R.eca_bwd_apply(c(d["dy"], dt), c(d["gate"], dt), c(d["dgap"], dt), case[4], mut)["dx"]}

    @staticmethod
    def bounds(case, kind):
        d = R.eca_apply_data(case, kind)
        return stored_bounds(R.eca_bwd_apply(d["dy"], d["gate"], d["dgap"], case[4]), case[4], "dx")


class StemFold:
    cases = [(cs, k) for cs in R.STEM_FOLD_CASES for k in R.KINDS]
    mutants = {"tap": lambda cs: cs[7] > 1, "share": None, "part": None}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, ipe, cout, coutp, cin, gld, cinp, ks = case
        d = R.stem_fold_data(case, kind)
        G, w = c(d["G"], dt), c(d["w"], dt)
        if flip:                                   # reversed filter rows: the ds sum in another order (dw: too few terms to matter)
            G, w = torch.cat([G[:, :, :cout].flip(2), G[:, :, cout:]], 2), w.flip(1)
        r = R.eca_stem_fold(G, c(d["gate"], dt), w, ipe, cout, cin, ks * ks, mut)
        return {"dw": (r["dw"].flip(1) if flip else r["dw"]).to(F64), "ds": r["ds"].to(F64)}

    @staticmethod
    def bounds(case, kind):
        E, ipe, cout, coutp, cin, gld, cinp, ks = case
        d = R.stem_fold_data(case, kind)
        r = R.eca_stem_fold(d["G"], d["gate"], d["w"], ipe, cout, cin, ks * ks)
        Ldw, Lds = R.stem_fold_chains(ipe, cout, ks * ks, gld)
        return {"dw": (Ldw + 8) * EPS * r["dw_abs"], "ds": (Lds + 8) * EPS * r["ds_abs"]}


class Nhwc:
    cases = [(cs, k) for cs in R.NHWC_CASES for k in R.KINDS]
    mutants = {"tap": None, "round2": lambda cs: cs[5] == F32}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        return {"dst": R.nchw_to_nhwc(R.nhwc_data(case, kind)["src"], case[4], case[5], mut)["dst"]}

    @classmethod
    def bounds(cls, case, kind):
        return zero_like(cls.run(case, kind, F64))


ACT_SMALL = [cs for cs in R.ACT_CASES if cs[0] < 100000]


class ActFwd:
    cases = [(cs, k) for cs in ACT_SMALL for k in R.KINDS]
    mutants = {"tap": lambda cs: cs[2] > 0 and cs[0] > 64 and cs[1] != R.ACT_TANH, "round2": lambda cs: cs[4] == F32 and cs[1] in (0, 1, 2)}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        n, act, p, seed, dtype = case
        return {"y": R.act_fwd(c(R.act_data(case, kind)["x"], dt), act, p, seed, dtype, mut)["y"]}

    @staticmethod
    def bounds(case, kind):
        n, act, p, seed, dtype = case
        r = R.act_fwd(R.act_data(case, kind)["x"], act, p, seed, dtype)
        return stored_bounds(r, dtype, "y", extra=r["allow"])


class ActBwd:
    cases = [(cs, k) for cs in ACT_SMALL for k in R.KINDS]
    mutants = {"tap": lambda cs: cs[2] > 0 and cs[1] >= R.ACT_ELU and cs[0] > 64, "last": lambda cs: cs[2] > 0 and cs[1] in (0, 3) and cs[0] > 64,
               "round2": lambda cs: cs[4] == F32 and cs[0] > 64}

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        n, act, p, seed, dtype = case
        d = R.act_data(case, kind)
        return {"dx": R.act_bwd(c(d["dy"], dt), c(d["y"], dt), act, p, dtype, mut)["dx"]}

    @staticmethod
    def bounds(case, kind):
        n, act, p, seed, dtype = case
        d = R.act_data(case, kind)
        return stored_bounds(R.act_bwd(d["dy"], d["y"], act, p, dtype), dtype, "dx")


GATE = [(cs, k) for cs in R.GATE_CASES for k in R.KINDS]


class GateFwd:
    cases = GATE
    mutants = {"G": lambda cs: R.gate_G(cs[0]) > cs[0] and not cs[2] & 2}
    lattice_applies = staticmethod(lambda cs: not cs[2] & 1)            # (with the ReLU the lattice's maximum is 256: a dead lane adds nothing)

    @staticmethod
    def run(case, kind, dt, mut="", flip=False):
        E, B, ar, shared, dtype = case
        d = R.gate_data(case, kind)
        r = R.gate_fwd(c(d["head"], dt), c(d["spd"], dt), B, E, ar, shared, mut)
        return {n: R.round_to(r[n].to(F64), F32) if kind == "lattice" else r[n].to(F64) for n in ("probs", "mean", "std", "speeds")}

    @staticmethod
    def bounds(case, kind):
        E, B, ar, shared, dtype = case
        d = R.gate_data(case, kind)
        r = R.gate_fwd(d["head"], d["spd"], B, E, ar, shared)
        return {"probs": r["probs_bound"], "std": r["std_bound"], "mean": 0 * r["mean"], "speeds": 0 * r["speeds"]}


class GateBwd:
    cases = GATE
    big = staticmethod(lambda cs: cs[0] > 1 and cs[0] * cs[1] >= 15)                # enough elements for every branch to occur
    mutants = {"G": lambda cs: GateBwd.big(cs) and not cs[2] & 2, "last": lambda cs: GateBwd.big(cs) and cs[2] & 1 and (cs[0] - R.pow2ceil(cs[0]) // 2) * cs[1] >= 8,
               "round2": lambda cs: GateBwd.big(cs) and cs[4] == F32 and not cs[2] & 2}

    @staticmethod
    def args(case, kind, dt):
        E, B, ar, shared, dtype = case
        d = R.gate_data(case, kind)
        return [c(d[n], dt) for n in ("head", "probs", "dprobs", "dmean", "dstd", "dspeeds")] + [B, E, ar, shared, d["rows"], d["ld"], R.SPD_LD, dtype]

    @classmethod
    def run(cls, case, kind, dt, mut="", flip=False):
        r = R.gate_bwd(*cls.args(case, kind, dt), mut)
        return {"dhead": torch.nan_to_num(r["dhead"]), "dspd": torch.nan_to_num(r["dspd"])}

    @classmethod
    def bounds(cls, case, kind):
        r = R.gate_bwd(*cls.args(case, kind, F64))
        z = torch.zeros_like(r["mag"])
        G = R.gate_G(case[0])
        return {"dhead": z if case[4] == BF16 else R.stored_bound(torch.nan_to_num(r["dhead_raw"]), r["mag"], r["allow"], int(math.log2(G))),
                "dspd": 0 * torch.nan_to_num(r["dspd"])}


LOSS_OUT = ("loss", "loglik", "dprobs", "dmean", "dstd", "dspeeds")


class MoeLoss:
    cases = [(cs, k) for cs in R.LOSS_CASES for k in R.loss_kinds(cs)]
    mutants = {"clampgrad": lambda cs: cs[0] > 1, "nohw": lambda cs: cs[0] > 1 and not cs[2]}
    lattice_mutants = ("nohw",)

    @staticmethod
    def args(case, kind, dt):
        E, B, shared = case
        d = R.loss_data(case, kind)
        return [c(d[n], dt) for n in ("probs", "mean", "std", "speeds", "act", "tgt")] + [d["c"][0], d["c"][1], B, E, shared]

    @classmethod
    def run(cls, case, kind, dt, mut="", flip=False):
        r = R.moe_loss(*cls.args(case, kind, dt), mut)
        names = ("loss", "dspeeds") if kind == "lattice" else LOSS_OUT
        return {n: r[n].to(F64) for n in names}

    @classmethod
    def bounds(cls, case, kind):
        a = cls.args(case, kind, F64)
        return R.moe_loss_bounds(R.moe_loss(*a), *a)


KERNELS = {k.__name__: k for k in (Maxpool, GapPartial, GapFinish, GapBwd, EcaGate, EcaBwdSmall, EcaScale, EcaApply, StemFold, Nhwc,
                                   ActFwd, ActBwd, GateFwd, GateBwd, MoeLoss)}


# ---------------------------------------------------------------------------------------------------------------------------------
# generators and bounds

@pytest.mark.parametrize("name", KERNELS)
def test_lattice_is_exact_in_float32_in_two_orders(name):
    K = KERNELS[name]
    n = 0
    for case, kind in K.cases:
        if kind != "lattice":
            continue
        ref = K.run(case, kind, F64)
        for flip in (False, True):
            got = K.run(case, kind, F32, flip=flip)
            for out, r in ref.items():
                assert torch.equal(got[out], r) or bool((errof(got[out], r) == 0).all()), (name, R.case_id(case), out, flip)
        n += 1
    assert n > 0, "no lattice case"


@pytest.mark.parametrize("name", KERNELS)
def test_float32_reference_stays_within_the_bounds(name):
    """the bounds are not vacuous: the plain float32 CPU evaluation meets them (bfloat16 storage and max pooling: equality)"""
    K = KERNELS[name]
    worst = 0.0
    for case, kind in K.cases:
        if kind != "continuous":
            continue
        ref, got, b = K.run(case, kind, F64), K.run(case, kind, F32), K.bounds(case, kind)
        for out, r in ref.items():
            e = errof(got[out], r)
            bad = e > b[out]
            assert not bad.any(), (name, R.case_id(case), out, (e / b[out].clamp_min(1e-300)).max().item())
            worst = max(worst, (e / b[out].clamp_min(1e-300))[e > 0].max().item() if (e > 0).any() else 0.0)
    print(f"{name}: float32 on the CPU, max err / bound {worst:.3f}")


MUTANTS = [(n, m) for n, K in KERNELS.items() for m in K.mutants]


@pytest.mark.parametrize("name,mut", MUTANTS, ids=[f"{n}-{m}" for n, m in MUTANTS])
def test_mutant_is_caught(name, mut):
    """on every case the mutant applies to: not equal on the lattice, 16 times the bound on the continuous kind"""
    K = KERNELS[name]
    applies = K.mutants[mut] or (lambda cs: True)
    seen = set()
    for case, kind in K.cases:
        if not applies(case):
            continue
        if kind == "lattice" and (mut not in getattr(K, "lattice_mutants", K.mutants) or not getattr(K, "lattice_applies", applies)(case)):
            continue
        ref, got = K.run(case, kind, F64), K.run(case, kind, F64, mut)
        if kind == "lattice":
            assert any(bool((errof(got[o], r) > 0).any()) for o, r in ref.items()), (name, mut, R.case_id(case), "equal on the lattice")
        else:
            b = K.bounds(case, kind)
            ratio = max((errof(got[o], r) / b[o].clamp_min(1e-300)).max().item() for o, r in ref.items())
            assert ratio >= 16, (name, mut, R.case_id(case), ratio)
        seen.add(kind)
    assert "continuous" in seen and ("lattice" in seen or mut not in getattr(K, "lattice_mutants", K.mutants)), (name, mut, seen)


def test_continuous_inputs_keep_their_distance():
    """bfloat16 storage: no stored value within 2^-18 of its addends' absolute sum (plus twice the transcendental allowance) of a
    rounding boundary; moe_loss: no normalised probability within a factor 2^10 of either clamp, except the planted ones"""
    for K, key in ((GapFinish, "out"), (EcaScale, "y"), (EcaApply, "dx"), (ActFwd, "y"), (ActBwd, "dx")):
        for case, kind in K.cases:
            dtype = [v for v in case if isinstance(v, torch.dtype)][0]
            if kind == "continuous" and dtype == BF16:
                f32 = K.run(case, kind, F32)[key]
                assert torch.equal(f32, K.run(case, kind, F64)[key]), (K.__name__, R.case_id(case))
    for case in R.ECA_SCALE_CASES:
        E, ipe, H, W, C, shared, dtype = case
        d = R.eca_scale_data(case, "continuous")
        r = R.eca_scale(d["x"], d["gate"], ipe if shared else 0, dtype)
        assert not R.near_boundary(r["raw"], R.TOL * r["mag"], dtype).any()
    for case in R.LOSS_CASES:
        E, B, shared = case
        d = R.loss_data(case, "continuous")
        pn = d["probs"] / d["probs"].sum(1, keepdim=True)
        planted = torch.zeros_like(pn, dtype=torch.bool)
        if E > 1:
            planted[0, E - 1] = True
            assert pn[0, E - 1] < R.LOSS_EPS / 16
            assert (pn[~planted] > R.LOSS_EPS * 1024).all() and (pn < 1 - 2.0 ** -13).all()
        else:
            assert (pn == 1).all()
    for case in R.MAXPOOL_CASES:                     # four-term sums of dy are exact in float32: max pooling rounds nothing
        dy = R.maxpool_data(case, "continuous")["dy"]
        assert torch.equal(dy.to(BF16).to(F64), dy) and (dy.abs() >= 2.0 ** -6).all() and (dy.abs() < 8).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference itself

def test_reference_matches_torch():
    g = R.gen("torch")
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    # max pool and its gradient (no ties in randn data)
    x = rn(2, 7, 6, 4)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    dy = rn(*yr.shape)
    yr.backward(dy)
    f = R.maxpool_fwd(x)
    assert torch.equal(f["y"].permute(0, 3, 1, 2), yr.detach())
    assert torch.allclose(R.maxpool_bwd(dy.permute(0, 2, 3, 1), f["am"], 7, 6, F64)["dx"].permute(0, 3, 1, 2), xr.grad, atol=1e-14)
    # first maximum wins: a constant window reports its first in-bounds tap
    am = R.maxpool_fwd(torch.zeros(1, 3, 3, 1, dtype=F64))["am"].flatten().tolist()
    assert am == [4, 3, 1, 0]
    # ECA forward and backward against autograd, private and shared input
    for shared in (False, True):
        E, ipe, creal, C, H, W, k, nparts = 2, 3, 12, 16, 5, 4, 5, 3
        N, nx = E * ipe, ipe if shared else E * ipe
        xs = torch.zeros(nx, H, W, C, dtype=F64)
        xs[..., :creal] = rn(nx, H, W, creal)
        w, dyy = rn(E, k), torch.zeros(N, H, W, C, dtype=F64)
        dyy[..., :creal] = rn(N, H, W, creal)
        xr, wr = xs.clone().requires_grad_(True), w.clone().requires_grad_(True)
        outs = []
        for e in range(E):
            xe = (xr if shared else xr[e * ipe:(e + 1) * ipe])[..., :creal]
            gmean = xe.mean((1, 2))
            s = torch.sigmoid(F.conv1d(gmean[:, None], wr[e][None, None], padding=k // 2)[:, 0])
            outs.append(xe * s[:, None, None, :])
        yt = torch.cat(outs)
        yt.backward(dyy[..., :creal])
        sh = ipe if shared else 0
        part = R.gap_partial(xs, None, nparts, 0)["part"]
        gt = R.eca_gate(part, H * W, w, k, N, ipe, sh, C, creal)
        y = R.eca_scale(xs, gt["gate"], sh, F64)["y"]
        assert torch.allclose(y[..., :creal], yt.detach(), atol=1e-13) and (y[..., creal:] == 0).all()
        dot = R.gap_partial(dyy, xs, nparts, sh)["part"]
        bs = R.eca_bwd_small(dot, gt["gate"], gt["gapmean"], w, k, ipe, C, creal, 1.0)
        assert torch.allclose(bs["dw"], wr.grad, atol=1e-12)
        if not shared:
            dx = R.eca_bwd_apply(dyy, gt["gate"], bs["dgap"], F64)["dx"]
            assert torch.allclose(dx[..., :creal], xr.grad[..., :creal], atol=1e-13)
    # global average pool
    x = rn(3, 4, 5, 8)
    fin = R.gap_finish(R.gap_partial(x, None, 3, 0)["part"], 20, F64)["out"]
    assert torch.allclose(fin, x.mean((1, 2)), atol=1e-14)
    assert torch.allclose(R.gap_bwd(fin, 20, 8, 0, F64)["dx"], (fin / 20)[:, None].expand(-1, 20, -1))
    # stem fold: d/dW and d/dgate of sum(conv(x * gate, W) * dz) from per-image filter gradients
    E, ipe, cout, cin, taps = 2, 3, 5, 6, 9
    Gr, gate, w = rn(E * ipe, taps, 8, 8), rn(E * ipe, 8), rn(E, cout, cin, taps)
    gr, wr = gate.clone().requires_grad_(True), w.clone().requires_grad_(True)
    g4 = Gr[:, :, :cout, :cin].permute(0, 2, 3, 1)
    (wr.repeat_interleave(ipe, 0) * gr[:, None, :cin, None] * g4).sum().backward()
    sf = R.eca_stem_fold(Gr, gate, w, ipe, cout, cin, taps)
    assert torch.allclose(sf["dw"], wr.grad, atol=1e-12) and torch.allclose(sf["ds"], gr.grad, atol=1e-12)


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("E,ar", ((1, 0), (1, 2), (3, 1), (8, 0), (33, 1)))
def test_head_reference_matches_torch_distributions(E, ar, shared):
    import torch.distributions as D
    B, dtype = 5, F32
    case = (E, B, ar, shared, dtype)
    d = R.gate_data(case, "continuous")
    hr, sr = d["head"].clone().requires_grad_(True), d["spd"].clone().requires_grad_(True)
    comp, alpha = R.head_views(hr, B, E, shared)
    a = torch.relu(alpha) if ar & 1 else alpha
    probs_t = (a + 1.5) if ar & 2 else torch.softmax(a, 1)         # (raw mode: shifted to stay positive for Categorical)
    mean_t, std_t = comp[..., :2], F.elu(comp[..., 2:4]) + 1
    speeds_t = sr[:B, 0:1] if shared else sr[:E * B, 0].reshape(E, B).t()[..., None]
    act, tgt = torch.rand(B, 2, dtype=F64) * 2 - 1, torch.rand(B, dtype=F64)
    dist = D.MixtureSameFamily(D.Categorical(probs_t), D.Independent(D.Normal(mean_t, std_t), 1))
    ll_t = dist.log_prob(act)
    mse = F.mse_loss(speeds_t, (tgt[:, None] if shared else tgt[:, None, None]).expand_as(speeds_t)) / (1 if shared else E)
    loss_t = 0.75 * -ll_t.mean() + 0.25 * mse
    loss_t.backward()
    fw = R.gate_fwd(d["head"], d["spd"], B, E, ar, shared)
    probs = fw["probs"] + 1.5 if ar & 2 else fw["probs"]
    assert torch.allclose(probs, probs_t.detach(), atol=1e-14) and torch.allclose(fw["std"], std_t.detach(), atol=1e-14)
    assert torch.equal(fw["speeds"], speeds_t.detach())
    ls = R.moe_loss(probs, fw["mean"], fw["std"], fw["speeds"], act, tgt, 0.75, 0.25, B, E, shared)
    assert torch.allclose(ls["loss"], loss_t.detach().reshape(1), atol=1e-13) and torch.allclose(ls["loglik"], ll_t.detach(), atol=1e-13)
    bw = R.gate_bwd(d["head"], fw["probs"], ls["dprobs"], ls["dmean"], ls["dstd"], ls["dspeeds"], B, E, ar, shared, d["rows"], d["ld"],
                    R.SPD_LD, F64)
    assert torch.allclose(torch.nan_to_num(bw["dhead"]), hr.grad, atol=1e-12)
    assert torch.allclose(torch.nan_to_num(bw["dspd"]), sr.grad, atol=1e-12)


def test_loss_clamp_and_null_gradients():
    """a probability below 2^-23 after normalisation: clamped, and its dprobs is zero; null gradients count as zeros"""
    p = torch.tensor([[0.5, 0.5 - 2.0 ** -30, 2.0 ** -30]], dtype=F64)
    one = torch.ones(1, 3, 2, dtype=F64)
    mu = torch.tensor([0.0, 0.5, -0.5], dtype=F64)[None, :, None] * one
    rest = (torch.zeros(1, 3, 1, dtype=F64), torch.zeros(1, 2, dtype=F64), torch.zeros(1, dtype=F64), 1.0, 0.0, 1, 3, False)
    r, kept = R.moe_loss(p, mu, one, *rest), R.moe_loss(p, mu, one, *rest, "clampgrad")
    assert r["clamped"].tolist() == [[False, False, True]] and r["dprobs"][0, 0] != 0
    assert r["dprobs"][0, 2] == 0 and kept["dprobs"][0, 2] != 0
    d = R.gate_data((3, 5, 1, False, F32), "continuous")
    full = R.gate_bwd(d["head"], d["probs"], 0 * d["dprobs"], d["dmean"], d["dstd"], d["dspeeds"], 5, 3, 1, False, d["rows"], d["ld"], 4, F32)
    null = R.gate_bwd(d["head"], d["probs"], None, d["dmean"], d["dstd"], d["dspeeds"], 5, 3, 1, False, d["rows"], d["ld"], 4, F32)
    assert torch.equal(torch.nan_to_num(full["dhead"]), torch.nan_to_num(null["dhead"]))


def test_activation_and_hash_reference():
    # the hash against a scalar transcription of csrc/common.h in Python integers
    def scalar(seed, idx):
        m = (1 << 64) - 1
        z = (seed + idx * 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return (z >> 40) / 16777216.0
    for seed in R.SEEDS + (0, (1 << 64) - 1):
        u = R.hash_uniform(seed, 1000)
        assert u.tolist() == [scalar(seed, i) for i in range(1000)]
        assert 0.45 < (u >= 0.5).to(F64).mean() < 0.55
    x = torch.linspace(-4, 4, 257, dtype=F64)
    for act, fn in ((R.ACT_RELU, torch.relu), (R.ACT_ELU, F.elu), (R.ACT_TANH, torch.tanh), (R.ACT_SIGMOID, torch.sigmoid)):
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        dy = torch.cos(x)
        y.backward(dy)
        assert torch.allclose(R.act_fwd(x, act, 0.0, 0, F64)["y"], y.detach(), atol=1e-15)
        assert torch.allclose(R.act_bwd(dy, y.detach(), act, 0.0, F64)["dx"], xr.grad, atol=1e-14)
        # inverted dropout: the kept elements scaled by 2, the gradient likewise
        f = R.act_fwd(x, act, 0.5, 7, F64)
        assert torch.equal(f["y"], torch.where(f["keep"], 2 * y.detach(), torch.zeros_like(x)))
        b = R.act_bwd(dy, f["y"], act, 0.5, F64)["dx"]
        live = f["keep"] & (f["y"] != 0)
        assert torch.allclose(b[live], 2 * xr.grad[live], atol=1e-14) and (b[~f["keep"]] == 0).all()


def test_transcendental_constants_are_twice_the_measured_error():
    for name, t in (("exp", R.T_EXP), ("expm1", R.T_EXPM1), ("tanh", R.T_TANH), ("log", R.T_LOG)):
        assert t == max(1, math.ceil(2 * R.MEASURED[name])), name
        assert R.MEASURED[name] <= 4, "a device function more than 4 units off is a finding, not a tolerance"


# ---------------------------------------------------------------------------------------------------------------------------------
# the case tables reach the code

def test_case_tables_cover_the_launch_code():
    # every route of pmoe_nchw_to_nhwc, each with a full tile, a partial tile and a tile boundary, in both dtypes, C = Cp and C < Cp
    seen = {}
    for B, C, H, W, Cp, dtype in R.NHWC_CASES:
        route = R.nhwc_route(B, C, H, W, Cp)
        full, part = R.nhwc_tiles(H * W, route)
        seen.setdefault((route, dtype), set()).update({("full", full > 0), ("partial", part > 0), ("only partial", full == 0),
                                                       ("exact", part == 0 and full > 0), ("B", B), ("padded", C < Cp)})
    for d in R.DTYPES:
        for route in ("tiled256", "tiled64"):
            assert {("full", True), ("partial", True), ("only partial", True), ("exact", True), ("B", 1), ("B", 3), ("padded", True),
                    ("padded", False)} <= seen[(route, d)], (route, d)
        assert ("plain", d) in seen
    assert {cs[4] for cs in R.NHWC_CASES} == {16, 32, 48, 240, 256}
    # every G of the gate kernels and of the loss; a batch smaller than, and one sample larger than, one pass
    for cases in (R.GATE_CASES, R.LOSS_CASES):
        assert {R.gate_G(cs[0]) for cs in cases} == {1, 4, 8, 64}
        for E in (1, 3, 8, 33, 64):
            Bs = {cs[1] for cs in cases if cs[0] == E}
            assert {1, 5, 256 // R.gate_G(E) + 1} <= Bs
    assert any(cs[2] & 2 and cs[0] == 1 for cs in R.GATE_CASES) and any(cs[2] == 0 and cs[0] == 1 for cs in R.GATE_CASES)
    for shared in (False, True):
        for d in R.DTYPES:
            assert any(cs[3] == shared and cs[4] == d and cs[2] & 1 for cs in R.GATE_CASES)
    # gap_partial: idle lanes, RL = 1, CV = 1, empty and ragged partitions, both sharing forms
    geo = {(R.stream_geometry(cs[4], cs[5]), cs[5]) for cs in R.GAP_PARTIAL_CASES}
    for d in R.DTYPES:
        assert ((1, 256), d) in geo and ((256, 1), d) in geo and any(256 % cv for (cv, rl), dd in geo if dd == d)
    assert any(R.nparts_of(cs[6], cs[2] * cs[3]) > cs[2] * cs[3] for cs in R.GAP_PARTIAL_CASES)
    assert any((cs[2] * cs[3]) % R.cdiv(cs[2] * cs[3], R.nparts_of(cs[6], cs[2] * cs[3])) for cs in R.GAP_PARTIAL_CASES)
    assert {cs[7] for cs in R.GAP_PARTIAL_CASES} == {"a", "ab", "ab_shared"}
    # each grid-stride loop
    ve = R.ve
    assert any(R.grid_stride_entered(cs[1] * cs[2] * cs[3] // ve(cs[6]), R.GRID_CAPS["gap_bwd"]) for cs in R.GAP_BWD_CASES)
    assert any(R.grid_stride_entered(cs[0] * cs[1], R.GRID_CAPS["gap_finish"]) for cs in R.GAP_FINISH_CASES)
    assert any(R.grid_stride_entered(cs[2] * cs[3] * cs[4] // ve(cs[6]), R.GRID_CAPS["eca_scale"]) for cs in R.ECA_SCALE_CASES)
    assert any(R.grid_stride_entered(cs[1] * cs[2] * cs[3] // ve(cs[4]), R.GRID_CAPS["eca_bwd_apply"]) for cs in R.ECA_APPLY_CASES)
    assert any(R.grid_stride_entered(cs[0] * cs[2], R.GRID_CAPS["pad_rows"]) for cs in R.PAD_ROWS_CASES)
    assert any(R.grid_stride_entered(cs[0] // ve(cs[4]), R.GRID_CAPS["act"]) for cs in R.ACT_CASES)
    # ECA: every k, every (creal, C), both input forms; stem fold: both row lengths
    assert {cs[4] for cs in R.ECA_CASES} == {1, 3, 5, 9}
    assert {(cs[3], cs[2]) for cs in R.ECA_CASES} == {(12, 16), (138, 144), (64, 64), (512, 512), (1000, 1024)}
    assert {cs[7] for cs in R.ECA_CASES} == {False, True} and {cs[5] for cs in R.ECA_CASES} == {1, 3}
    assert {cs[5] for cs in R.STEM_FOLD_CASES} == {16, 144} and {cs[7] for cs in R.STEM_FOLD_CASES} == {1, 3}
    assert {cs[1] for cs in R.ACT_CASES} == set(range(5)) and {cs[3] for cs in R.ACT_CASES if cs[2] > 0} == set(R.SEEDS)
