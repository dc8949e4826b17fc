"""The float64 BatchNorm reference (tests/bn_ref.py) checked against torch's own batch_norm / ReLU / max_pool2d / mean chain and
its autograd, and the input generators checked for everything tests/test_bn_gpu.py assumes of them.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

F64, F32, BF16 = R.F64, R.F32, R.BF16
ALL_CASES = R.CASES + R.POOL_CASES + R.GAP_CASES
ALL_IDS = [R.case_id(c) for c in ALL_CASES]
# (E, ipe, H, W, C): the shapes of the GPU cases at C = 8 (the reference has no channel-count paths), every nparts of the GPU tests
TORCH_SHAPES = [(3, 1, 7, 11, 8), (2, 2, 5, 3, 8), (1, 1, 3, 5, 8), (2, 3, 9, 9, 8), (1, 2, 4, 4, 8), (1, 1, 2, 2, 8),
                (2, 3, 6, 2, 8), (1, 2, 4, 10, 8), (2, 2, 1, 5, 8)]


def relerr(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", TORCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_chain_matches_torch_and_autograd(shape):
    E, B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    N, rpe, eps, mom = E * B, B * H * W, 1e-5, 0.1
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, res, dy = rn(N, H, W, C) * 1.5 + 0.3, rn(N, H, W, C), rn(N, H, W, C)
    gamma, beta, rm, rv = 1 + 0.1 * rn(E, C), 0.1 * rn(E, C), 0.05 * rn(E, C), 1 + 0.1 * rn(E, C).abs()
    on = torch.ones(E, dtype=torch.bool)
    for nparts in sorted({1, 4, rpe + 1, *R.FIN_NPARTS}):
        cs = R.colstats(x.reshape(-1, C), rpe, E, C, C, 0, nparts)
        nmid = min(nparts, 128)
        mid = R.reduce_partials(cs["part"].reshape(E, nparts, 2 * C), nmid)["out"].reshape(E, nmid, 2, C)
        fin = R.bn_finalize(mid, rpe, gamma, beta, (rm, rv, on), mom, eps, True, cs["shiftc"])
        if nparts == 1:
            first = fin
        for n in ("mean", "var", "invstd", "scale", "rmean", "rvar"):          # partitioned == unpartitioned
            assert relerr(fin[n], first[n]) < 1e-9, (n, nparts)
    fin = first
    sc, sh, mu, istd = fin["scale"], fin["shift"], fin["mean"], fin["invstd"]
    ap = R.bn_apply(x, res, sc, sh, mu, E, True, F64)
    plain = R.bn_apply(x, None, sc, sh, mu, E, True, F64)
    nr = R.bn_bwd_reduce(dy, None, x, mu, istd, sc, sh, E, True, 4)
    for nparts in (1, 4, rpe + 1):
        br = R.bn_bwd_reduce(dy, ap["y"], x, mu, istd, sc, sh, E, True, nparts)
        bf = R.bn_bwd_finalize(br["part"], rpe)
        if nparts == 1:
            bf1 = bf
        for n in ("dbeta", "dgamma", "c1", "c2"):
            assert relerr(bf[n], bf1[n]) < 1e-9, (n, nparts)
    bf = bf1
    ba = R.bn_bwd_apply(dy, ap["y"], x, mu, istd, sc, sh, bf["c1"], bf["c2"], E, True, F64)
    nf = R.bn_bwd_finalize(nr["part"], rpe)
    na = R.bn_bwd_apply(dy, None, x, mu, istd, sc, sh, nf["c1"], nf["c2"], E, True, F64)
    gp = R.bn_apply_gap(x, sc, sh, mu, 4, B, True, F64)
    assert torch.equal(gp["y"], plain["y"])
    if H % 2 == 0 and W % 2 == 0:
        po = R.bn_apply_pool2(x, sc, sh, mu, E, True, F64)
        assert torch.equal(po["y"], plain["y"])
    for e in range(E):
        s = slice(e * B, (e + 1) * B)
        xr, rr = nchw(x[s]).clone().requires_grad_(True), nchw(res[s]).clone().requires_grad_(True)
        gr, br_ = gamma[e].clone().requires_grad_(True), beta[e].clone().requires_grad_(True)
        rme, rve = rm[e].clone(), rv[e].clone()
        yr = F.relu(F.batch_norm(xr, rme, rve, gr, br_, True, mom, eps) + rr)
        yr.backward(nchw(dy[s]))
        assert relerr(nchw(ap["y"][s]), yr.detach()) < 1e-10
        assert relerr(fin["rmean"][e], rme) < 1e-10 and relerr(fin["rvar"][e], rve) < 1e-10
        assert relerr(nchw(ba["dx"][s]), xr.grad) < 1e-10 and relerr(nchw(ba["gm"][s]), rr.grad) < 1e-10
        assert relerr(bf["dgamma"][e], gr.grad) < 1e-10 and relerr(bf["dbeta"][e], br_.grad) < 1e-10
        # no residual: the recomputed mask, pooling and the spatial mean
        x2 = nchw(x[s]).clone().requires_grad_(True)
        y2 = F.relu(F.batch_norm(x2, None, None, gamma[e], beta[e], True, mom, eps))
        y2.backward(nchw(dy[s]))
        assert relerr(nchw(plain["y"][s]), y2.detach()) < 1e-10 and relerr(nchw(na["dx"][s]), x2.grad) < 1e-10
        assert relerr(gp["part"][s].sum(1) / (H * W), y2.detach().mean((2, 3))) < 1e-10
        if H % 2 == 0 and W % 2 == 0:
            assert relerr(nchw(po["pooled"][s]), F.max_pool2d(y2.detach(), 2)) < 1e-10
        # eval mode reads the running buffers
        ev = R.bn_finalize(cs["part"], rpe, gamma, beta, (rm, rv, on), mom, eps, False, None)
        ye = R.bn_apply(x, None, ev["scale"], ev["shift"], ev["mean"], E, False, F64)["y"]
        assert relerr(nchw(ye[s]), F.batch_norm(nchw(x[s]), rm[e], rv[e], gamma[e], beta[e], False, mom, eps)) < 1e-10
    # gap_partial: sums of a and of a * b, private and shared b
    a = R.gap_partial(x, None, 4, 0)
    assert relerr(a["part"].sum(1), x.sum((1, 2))) < 1e-10
    ab = R.gap_partial(x, res[:B], 4, B)
    assert relerr(ab["part"].sum(1), (x * res[:B].repeat(E, 1, 1, 1)).sum((1, 2))) < 1e-10


def test_reference_edges():
    """count == 1, null tables, empty partitions and the channel window of the reference itself"""
    part = torch.tensor([[[[2.0], [5.0]], [[1.0], [4.5]]]], dtype=F64)                      # E 1, nparts 2, C 1
    rm, rv = torch.tensor([[1.0]], dtype=F64), torch.tensor([[3.0]], dtype=F64)
    f = R.bn_finalize(part, 1, None, None, (rm, rv, torch.tensor([True])), 0.5, 0.25, True, torch.tensor([[10.0]], dtype=F64))
    assert f["mean"].item() == 13.0 and f["var"].item() == 0.5 and f["scale"].item() == f["invstd"].item() and f["shift"].item() == 0
    assert f["rmean"].item() == 7.0 and f["rvar"].item() == 1.75                           # count 1: the biased variance
    f = R.bn_finalize(part, 1, None, None, (rm, rv, torch.tensor([False])), 0.5, 0.25, True, None)
    assert f["rmean"].item() == 1.0 and f["rvar"].item() == 3.0 and f["mean"].item() == 3.0
    x = torch.arange(12, dtype=F64).reshape(3, 4)                                          # 3 rows, ld 4, window [2, 4)
    c = R.colstats(torch.where(x % 4 < 2, float("nan"), x), 3, 1, 2, 4, 2, 4)
    assert c["part"][0, :, 0].tolist() == [[0, 0], [4, 4], [8, 8], [0, 0]] and c["shiftc"].tolist() == [[2, 3]]
    assert c["part"][0, :, 1].tolist() == [[0, 0], [16, 16], [64, 64], [0, 0]]
    r = R.reduce_partials(torch.arange(5, dtype=F64).reshape(1, 5, 1), 4)                  # per 2: rows 01 | 23 | 4 | -
    assert r["out"].flatten().tolist() == [1, 5, 4, 0]


def _two_orders(d, case):
    """every kernel formula in float32, once fused (addcmul = one rounding per multiply-add) and once multiply then add; and the
    same in float64"""
    E, dtype = case[0], case[5]
    out = {}
    for name, dt, fused in (("f64", F64, False), ("fused", F32, True), ("split", F32, False)):
        k = {n: t.to(dt)[:, None] for n, t in d["k"].items()}
        x, res, dy = (R.rows(d[n], E).to(dt) for n in ("x", "res", "dy"))
        fma = (lambda c, a, b: torch.addcmul(c, a, b)) if fused else (lambda c, a, b: a * b + c)
        u = x - k["mean"]
        pre = fma(k["shift"].expand_as(u), u, k["scale"])
        g = torch.where(pre > 0, dy, torch.zeros((), dtype=dt))
        Bx, K = -k["scale"] * k["invstd"] * k["c2"], -k["scale"] * k["c1"]
        dev = x - x[:, :1]
        t = {"pre": pre, "pre_res": pre + res, "g": g, "dev": dev,
             "dev2": fma(torch.zeros_like(dev), dev, dev),
             "gxhat": g * u * k["invstd"] if fused else g * (u * k["invstd"]),
             "dx": fma(fma(K.expand_as(u), u, Bx), g, k["scale"]) if fused else g * k["scale"] + (u * Bx + K),
             "ab": x * dy}
        out[name] = {n: v.to(F64) for n, v in t.items()}
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_lattice_inputs_make_float32_arithmetic_exact(case):
    E, B, H, W, C, dtype = case
    d = R.lattice_case(case)
    k = d["k"]
    t = _two_orders(d, case)
    unit = 2.0 ** R.LATTICE_G
    for n, ref in t["f64"].items():
        assert torch.equal(t["fused"][n], ref) and torch.equal(t["split"][n], ref), n
        assert ((ref * unit) == (ref * unit).round()).all(), f"{n}: not a multiple of 2^-{R.LATTICE_G}"
        # an accumulator never holds more than its (expert, channel)'s absolute sum
        assert (ref.abs().sum(1) * unit).max() < 2 ** 24, n
    # every stored tensor round-trips through the storage type
    for n in ("x", "res", "dy"):
        assert torch.equal(d[n].to(dtype).to(F64), d[n]), n
    for n in ("pre", "pre_res", "dx", "g"):
        assert torch.equal(t["f64"][n].to(F32).to(dtype).to(F64), t["f64"][n]), n
    for n, v in k.items():
        assert torch.equal(v.to(F32).to(F64), v), n
    # the planted elements: exactly on the ReLU edge and one step either side, by x and by the residual
    code = R.planted(case)
    pre, pre_res = t["f64"]["pre"], t["f64"]["pre_res"]
    step = (k["scale"] / 4)[:, None].expand_as(pre)
    for c_, v, s in ((1, pre, 0 * step), (2, pre, step), (3, pre, -step), (5, pre_res, 0 * step + 0), (6, pre_res, 0 * step + 0.125),
                     (7, pre_res, 0 * step - 0.125)):
        assert (code == c_).any() and torch.equal(v[code == c_], s[code == c_]), c_
    cs = R.colstats(d["x"].reshape(-1, C), B * H * W, E, C, C, 0, 1)
    assert (cs["part"][:, 0, :, R.ALL_EQUAL_CHANNEL] == 0).all()                 # variance 0
    assert (t["f64"]["dev"][:, :, R.EXTREME_CHANNEL] <= 0).all()                 # row 0 is the channel's maximum


@pytest.mark.parametrize("count", (1, 64))
@pytest.mark.parametrize("nparts", (1, 33, 129, 2048))
def test_finalize_lattice_is_exact_in_float32(nparts, count):
    E, C = 3, 40
    d = R.finalize_lattice(E, nparts, C, count, 7)
    part = d["part"]
    assert torch.equal((part * 4).round(), part * 4) and part.abs().max() < 2 ** 22
    assert torch.equal(part.to(F32).to(F64), part)
    on = torch.tensor([True, False, True])
    ref = R.bn_finalize(part, count, d["gamma"], d["beta"], (d["rmean"], d["rvar"], on), d["momentum"], d["eps"], True, d["shiftc"])
    assert torch.equal(ref["var"], d["var"])
    f32 = R.bn_finalize(part.to(F32), count, d["gamma"].to(F32), d["beta"].to(F32), (d["rmean"].to(F32), d["rvar"].to(F32), on),
                        d["momentum"], d["eps"], True, d["shiftc"].to(F32))
    for n in ("mean", "var", "rmean"):
        assert torch.equal(f32[n].to(F64), ref[n]), n
    s = ref["var"] + d["eps"]
    assert torch.equal(torch.log2(s) / 2, (torch.log2(s) / 2).round())           # a power of 4
    b = R.bn_bwd_finalize(part, count)
    for n in ("dbeta", "dgamma", "c1", "c2"):
        assert torch.equal(b[n].to(F32).to(F64), b[n]), n
    ev = R.bn_finalize(part, count, d["gamma"], d["beta"], (d["rmean"], d["rvar"], on), d["momentum"], d["eps"], False, None)
    s = ev["var"] + d["eps"]
    assert torch.equal(torch.log2(s) / 2, (torch.log2(s) / 2).round())


def _f32(d):
    return {"x": d["x"].to(F32), "res": d["res"].to(F32), "dy": d["dy"].to(F32), "k": {n: t.to(F32) for n, t in d["k"].items()}}


def _within(got, ref, ref_abs, L, what):
    err = (got.to(F64) - ref).abs()
    assert (err <= (L + 8) * R.EPS24 * ref_abs).all(), f"{what}: {(err / (R.EPS24 * ref_abs).clamp_min(1e-300)).max().item():.2f} > {L + 8}"


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_continuous_inputs_leave_nothing_ambiguous(case):
    """no ambiguous element is left, and the plain float32 evaluation of the reference formulas on the CPU meets every bound
    that tests/test_bn_gpu.py applies to the kernels"""
    E, B, H, W, C, dtype = case
    d = R.continuous_case(case)
    assert not R.forward_ambiguous(d, case).any() and not R.backward_ambiguous(d, case).any()
    for n in ("x", "res", "dy"):
        assert torch.equal(d[n].to(dtype).to(F64), d[n]), n
    for n, v in d["k"].items():
        assert torch.equal(v.to(F32).to(F64), v), n
    ch0 = R.rows(d["x"], E)[:, :, 0]
    assert B * H * W < 8 or (ch0.mean(1).abs() > 16 * ch0.std(1)).all()           # |mean| >> std
    f, k, kf = _f32(d), d["k"], _f32(d)["k"]
    rpe = B * H * W
    forms, forms32 = R.mask_forms(d, case), R.mask_forms(d, case)
    for name in NPARTS_ALL:
        nparts = R.nparts_of(name, rpe)
        L = R.chain_stream(rpe, nparts, C, dtype)
        a, b = R.colstats(d["x"].reshape(-1, C), rpe, E, C, C, 0, nparts), R.colstats(f["x"].reshape(-1, C), rpe, E, C, C, 0, nparts)
        _within(b["part"], a["part"], a["abs"], L, "colstats")
        for form, (relu, y) in forms.items():
            y32 = None if y is None else y.to(F32)
            a = R.bn_bwd_reduce(d["dy"], y, d["x"], k["mean"], k["invstd"], k["scale"], k["shift"], E, relu, nparts)
            b = R.bn_bwd_reduce(f["dy"], y32, f["x"], kf["mean"], kf["invstd"], kf["scale"], kf["shift"], E, relu, nparts)
            _within(b["part"], a["part"], a["abs"], L, f"bn_bwd_reduce {form}")
            assert torch.equal(b["gmask"].to(F64), a["gmask"])
        npg = R.nparts_of(name, H * W)
        Lg = R.chain_stream(H * W, npg, C, dtype)
        for bb, ipe in ((None, 0), (d["dy"], 0), (d["dy"][:B], B)):
            a = R.gap_partial(d["x"], bb, npg, ipe)
            b = R.gap_partial(f["x"], None if bb is None else bb.to(F32), npg, ipe)
            _within(b["part"], a["part"], a["abs"], Lg, "gap_partial")
    half_ulp = lambda v: v.abs() * (2.0 ** -8 if dtype == BF16 else R.EPS24)
    for res in (None, "res"):
        for relu in (False, True):
            a = R.bn_apply(d["x"], None if res is None else d["res"], k["scale"], k["shift"], k["mean"], E, relu, dtype)
            b = R.bn_apply(f["x"], None if res is None else f["res"], kf["scale"], kf["shift"], kf["mean"], E, relu, dtype)
            if dtype == BF16:
                assert torch.equal(b["y"], a["y"]), "bn_apply"
            else:
                assert ((b["y"] - a["y"]).abs() <= 8 * R.EPS24 * a["mag"] + half_ulp(a["y"])).all(), "bn_apply"
    for form, (relu, y) in forms.items():
        a = R.bn_bwd_apply(d["dy"], y, d["x"], k["mean"], k["invstd"], k["scale"], k["shift"], k["c1"], k["c2"], E, relu, dtype)
        b = R.bn_bwd_apply(f["dy"], None if y is None else y.to(F32), f["x"], kf["mean"], kf["invstd"], kf["scale"], kf["shift"],
                           kf["c1"], kf["c2"], E, relu, dtype)
        if dtype == BF16:
            assert torch.equal(b["dx"], a["dx"]), f"bn_bwd_apply {form}"
        else:
            assert ((b["dx"] - a["dx"]).abs() <= 8 * R.EPS24 * a["mag"] + half_ulp(a["dx"])).all(), f"bn_bwd_apply {form}"
        assert torch.equal(b["gm"].to(F64), a["gm"])


NPARTS_ALL = R.NPARTS


@pytest.mark.parametrize("kind", ("lattice", "continuous"))
def test_finalize_rows_and_bounds(kind):
    """the synthetic partial rows: float32 values, no two rows of one channel alike, the continuous variance away from its clamp;
    and the float32 CPU evaluation of the finalize formulas lies within finalize_bounds"""
    for nparts, C, count in ((1, 8, 64), (97, 40, 1), (129, 32, 64), (2048, 64, 64)):
        E = 3
        d = R.finalize_data(kind, E, nparts, C, count, 11)
        part = d["part"]
        assert torch.equal(part.to(F32).to(F64), part)
        if nparts > 1 and kind == "lattice":
            srt = part[:, :-1].abs().sort(1).values
            assert (srt[:, 1:] != srt[:, :-1]).all() and (part[:, :-1] != 0).all()
        on = torch.tensor([True, False, True])
        for training in (True, False):
            ref = R.bn_finalize(part, count, d["gamma"], d["beta"], (d["rmean"], d["rvar"], on), d["momentum"], d["eps"], training,
                                d["shiftc"] if training else None)
            if kind == "continuous" and training:
                assert (ref["var"] >= 0.7 * part[:, :, 1].sum(1) / count).all()
            f = lambda t: t.to(F32)
            got = R.bn_finalize(part, count, d["gamma"], d["beta"], (d["rmean"], d["rvar"], on), d["momentum"], d["eps"],
                                training, d["shiftc"] if training else None)
            # float32 from the first rounding the kernel makes: mean and var are cast, the rest is float32 arithmetic
            mean32, var32 = f(got["mean"]), f(got["var"])
            is32 = torch.rsqrt(var32 + torch.tensor(d["eps"], dtype=F32))
            bound = R.finalize_bounds(ref, d, count, training, True)
            assert ((mean32.to(F64) - ref["mean"]).abs() <= bound["mean"]).all()
            assert ((is32.to(F64) - ref["invstd"]).abs() <= bound["invstd"]).all()
            assert (((f(d["gamma"]) * is32).to(F64) - ref["scale"]).abs() <= bound["scale"]).all()
            if training:
                m = torch.tensor(d["momentum"], dtype=F32)
                rm32 = (1 - m) * f(d["rmean"]) + m * mean32
                rv32 = (1 - m) * f(d["rvar"]) + m * f(got["unb"])
                o = on[:, None]
                assert ((rm32.to(F64) - ref["rmean"]).abs() <= bound["rmean"])[o.expand_as(rm32)].all()
                assert ((rv32.to(F64) - ref["rvar"]).abs() <= bound["rvar"])[o.expand_as(rv32)].all()
