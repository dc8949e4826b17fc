"""Every stand-alone BatchNorm pass of csrc/elementwise.hip against the float64 reference of its own operation (tests/bn_ref.py),
at the smallest shapes that reach each edge: one row per expert, a ragged last partition, more partitions than rows, one channel
vector per row (256 rows in flight) and 256 of them (one row in flight), idle lanes, channel windows, every fold path of the
finalize kernels up to 2048 partial rows.

Two kinds of input (tests/test_bn_cpu.py checks on the CPU what is assumed of them here):
  lattice     every input, constant and intermediate is a multiple of 2^-4 small enough that float32 arithmetic is EXACT in any
              order, fused or not: every output must equal the reference (the sign of a zero in masked gradients apart), through
              pre-activations planted exactly on the ReLU edge and one step either side, a constant channel and a channel whose
              first row is its maximum.  Of the finalize kernels only rsqrtf is inexact there.
  continuous  randn data, scaled and offset, redrawn where a float32 evaluation could land on the other side of a ReLU or of a
              bfloat16 rounding boundary; the bounds follow from float32 rounding alone:
                sums      |got - ref| <= (L + 8) 2^-24 sum|term| per partition row, L = the longest chain of sequential float32
                          additions of the launch (bn_ref.chain_stream, chain_reduce)
                finalize  the fold is in double: bn_ref.finalize_bounds
                stored    bfloat16: equal to the rounded reference; float32: within 8 2^-24 sum|addends| + half a unit in the
                          last place
Outputs are NaN- or sentinel-filled before each launch; every kernel gets the REFERENCE's results of the kernels before it.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests import bn_ref as R  # noqa: E402

DEV = "cuda"
F64, F32, BF16 = R.F64, R.F32, R.BF16
EPS = R.EPS24
KINDS = ("lattice", "continuous")
IDS = [R.case_id(c) for c in R.CASES]
SENTINEL = -77.0


def ids(cases):
    return [R.case_id(c) for c in cases]


@functools.lru_cache(maxsize=None)
def setup(case, kind):
    """inputs on the device, computed once per (case, kind) and never modified"""
    E, B, H, W, C, dtype = case
    d = R.case_data(case, kind)
    s = dict(d)
    for n in ("x", "res", "dy"):
        s[n + "d"] = d[n].to(dtype).to(DEV)
        assert torch.equal(s[n + "d"].cpu().to(F64), d[n])
    s["kd"] = {n: t.to(F32).to(DEV) for n, t in d["k"].items()}
    for n, t in d["k"].items():
        assert torch.equal(s["kd"][n].cpu().to(F64), t)
    s["forms"] = R.mask_forms(d, case)
    return s


def nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def on_dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


def same(got, ref, what):
    """exact equality of every value (the sign of a zero apart: a masked gradient is +0 or -0 by how the mask is applied)"""
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = ~(got == ref)
    if bad.any():
        i = bad.flatten().nonzero()[:6, 0]
        pairs = list(zip(got.flatten()[i].tolist(), ref.flatten()[i].tolist()))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first (got, ref): {pairs}; "
                             f"indices {[tuple(int(v) for v in torch.unravel_index(j, got.shape)) for j in i]}")


def check_sum(got, ref, ref_abs, L, kind, what):
    """partition rows: exact on the lattice, (L + 8) 2^-24 sum|term| else; an empty partition is zero in both"""
    got = got.detach().cpu().to(F64)
    assert not torch.isnan(got).any(), f"{what}: unwritten partition rows"
    err = (got - ref).abs()
    print(f"{what}: max |err| {err.max().item():.3e}, max err / (2^-24 sum|term|) "
          f"{(err / (EPS * ref_abs).clamp_min(1e-300)).max().item():.2f}, L {L}")
    if kind == "lattice":
        same(got, ref, what)
    else:
        assert (err <= (L + 8) * EPS * ref_abs).all(), what


def check_stored(got, ref, mag, kind, dtype, what):
    """a stored activation or gradient: exact on the lattice and in bfloat16 (the generator left no element near a rounding
    boundary), 8 2^-24 sum|addends| + half a unit in the last place in float32"""
    got = got.detach().cpu().to(F64)
    assert not torch.isnan(got).any(), f"{what}: unwritten elements"
    if kind == "lattice" or dtype == BF16:
        same(got, ref, what)
        return
    err = (got - ref).abs()
    bound = 8 * EPS * mag + ref.abs() * EPS
    print(f"{what}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all(), what


# ---------------------------------------------------------------------------------------------------------------------------------
# colstats

@pytest.mark.parametrize("parts", R.NPARTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_colstats_matches_reference(case, kind, parts):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    rpe = B * H * W
    nparts = R.nparts_of(parts, rpe)
    L = R.chain_stream(rpe, nparts, C, dtype)
    for use_shiftc in (True, False):
        ref = R.colstats(s["x"].reshape(-1, C), rpe, E, C, C, 0, nparts, use_shiftc)
        part, shiftc = nan(E, nparts, 2, C), nan(E, C)
        ops.colstats(rpe, s["xd"], E, C, part, nparts, shiftc=shiftc if use_shiftc else None)
        torch.cuda.synchronize()
        check_sum(part, ref["part"], ref["abs"], L, kind, f"colstats shiftc={use_shiftc}")
        if use_shiftc:
            same(shiftc, ref["shiftc"], "shiftc")                   # a copy of row 0 in both kinds
        else:
            assert torch.isnan(shiftc).all()


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_colstats_of_a_channel_window(case, kind, window):
    """the form Engine._colsum uses (bias gradients, concatenation buffers): everything outside the window is NaN"""
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    rpe, nparts = B * H * W, 4
    ld, coff = R.window_of(window, C, dtype)
    buf = torch.full((E * rpe, ld), float("nan"), dtype=F64)
    buf[:, coff:coff + C] = s["x"].reshape(-1, C)
    L = R.chain_stream(rpe, nparts, C, dtype)
    for use_shiftc in (False, True):
        ref = R.colstats(buf, rpe, E, C, ld, coff, nparts, use_shiftc)
        part, shiftc = nan(E, nparts, 2, C), nan(E, C)
        ops.colstats(rpe, buf.to(dtype).to(DEV), E, C, part, nparts, ld=ld, coff=coff, shiftc=shiftc if use_shiftc else None)
        torch.cuda.synchronize()
        check_sum(part, ref["part"], ref["abs"], L, kind, f"colstats window {window} shiftc={use_shiftc}")
        if use_shiftc:
            same(shiftc, ref["shiftc"], "shiftc")


@pytest.mark.parametrize("parts", R.NPARTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bn_bwd_reduce_matches_reference(case, kind, parts):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    rpe = B * H * W
    nparts = R.nparts_of(parts, rpe)
    L = R.chain_stream(rpe, nparts, C, dtype)
    for form, (relu, y) in s["forms"].items():
        ref = R.bn_bwd_reduce(s["dy"], y, s["x"], k["mean"], k["invstd"], k["scale"], k["shift"], E, relu, nparts)
        for with_gmask in (True, False):
            part = nan(E, nparts, 2, C)
            gmask = nan(*s["x"].shape, dtype=dtype) if with_gmask else None
            ops.bn_bwd_reduce(s["dyd"], on_dev(y, dtype), s["xd"], kd["mean"], kd["invstd"], kd["scale"], kd["shift"], rpe, E, C, relu,
                              part, nparts, gmask=gmask)
            torch.cuda.synchronize()
            check_sum(part, ref["part"], ref["abs"], L, kind, f"bn_bwd_reduce {form}")
            if with_gmask:
                same(gmask, ref["gmask"], f"gmask {form}")          # a copy of dy or a zero in both kinds


# ---------------------------------------------------------------------------------------------------------------------------------
# apply passes

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bn_apply_matches_reference(case, kind):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    for with_res in (False, True):
        for relu in (False, True):
            ref = R.bn_apply(s["x"], s["res"] if with_res else None, k["scale"], k["shift"], k["mean"], E, relu, dtype)
            y = nan(*s["x"].shape, dtype=dtype)
            ops.bn_apply(s["xd"], s["resd"] if with_res else None, y, kd["scale"], kd["shift"], kd["mean"], B * H * W, E, C, relu)
            torch.cuda.synchronize()
            check_stored(y, ref["y"], ref["mag"], kind, dtype, f"bn_apply res={with_res} relu={relu}")


def window_buffer(case, window):
    E, B, H, W, C, dtype = case
    ld, coff = R.window_of(window, C, dtype)
    inside = torch.zeros(ld, dtype=torch.bool)
    inside[coff:coff + C] = True
    return torch.full((E * B, H, W, ld), SENTINEL, dtype=dtype, device=DEV), coff, inside


def check_window(buf, inside, ref, mag, kind, dtype, what):
    buf = buf.cpu()
    assert (buf[..., ~inside] == SENTINEL).all(), f"{what}: wrote outside its channel window"
    check_stored(buf[..., inside], ref, mag, kind, dtype, what)


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bn_apply_into_a_channel_window(case, kind, window):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    for with_res, relu in ((True, True), (False, False)):
        ref = R.bn_apply(s["x"], s["res"] if with_res else None, k["scale"], k["shift"], k["mean"], E, relu, dtype)
        buf, coff, inside = window_buffer(case, window)
        ops.bn_apply(s["xd"], s["resd"] if with_res else None, buf, kd["scale"], kd["shift"], kd["mean"], B * H * W, E, C, relu,
                     y_coff=coff)
        torch.cuda.synchronize()
        check_window(buf, inside, ref["y"], ref["mag"], kind, dtype, f"bn_apply window {window} res={with_res}")


@pytest.mark.parametrize("window", ("dense",) + R.WINDOWS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=ids(R.POOL_CASES))
def test_bn_apply_pool2_matches_reference(case, kind, window):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    for relu in (True, False):
        ref = R.bn_apply_pool2(s["x"], k["scale"], k["shift"], k["mean"], E, relu, dtype)
        pooled = nan(E * B, H // 2, W // 2, C, dtype=dtype)
        if window == "dense":
            y = nan(*s["x"].shape, dtype=dtype)
            ops.bn_apply_pool2(s["xd"], y, pooled, kd["scale"], kd["shift"], kd["mean"], B, E, C, relu)
            torch.cuda.synchronize()
            check_stored(y, ref["y"], ref["mag"], kind, dtype, "bn_apply_pool2 y")
        else:
            buf, coff, inside = window_buffer(case, window)
            ops.bn_apply_pool2(s["xd"], buf, pooled, kd["scale"], kd["shift"], kd["mean"], B, E, C, relu, y_coff=coff)
            torch.cuda.synchronize()
            check_window(buf, inside, ref["y"], ref["mag"], kind, dtype, f"bn_apply_pool2 window {window}")
        # the maximum of four stored values, each within its own bound: the largest of the four bounds covers it
        check_stored(pooled, ref["pooled"], R.pool2(ref["mag"]), kind, dtype, "bn_apply_pool2 pooled")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bn_bwd_apply_matches_reference(case, kind):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    for form, (relu, y) in s["forms"].items():
        ref = R.bn_bwd_apply(s["dy"], y, s["x"], k["mean"], k["invstd"], k["scale"], k["shift"], k["c1"], k["c2"], E, relu, dtype)
        for with_gm in (True, False):
            dx = nan(*s["x"].shape, dtype=dtype)
            gm = nan(*s["x"].shape, dtype=dtype) if with_gm else None
            ops.bn_bwd_apply(s["dyd"], on_dev(y, dtype), s["xd"], kd["mean"], kd["invstd"], kd["scale"], kd["shift"], kd["c1"],
                             kd["c2"], dx, gm, B * H * W, E, C, relu)
            torch.cuda.synchronize()
            check_stored(dx, ref["dx"], ref["mag"], kind, dtype, f"bn_bwd_apply dx {form}")
            if with_gm:
                same(gm, ref["gm"], f"bn_bwd_apply gm {form}")


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_the_three_mask_forms_agree_on_the_relu_edge(case):
    """lattice data with pre-activations planted at exactly 0 and one step either side: the mask from the saved output, the mask
    recomputed from x and the pre-masked gradient with relu off give the same gmask, partial rows and dx -- the reference's"""
    E, B, H, W, C, dtype = case
    s = setup(case, "lattice")
    k, kd = s["k"], s["kd"]
    rpe, nparts = B * H * W, 4
    code = R.planted(case).reshape(s["x"].shape)
    y = R.bn_apply(s["x"], None, k["scale"], k["shift"], k["mean"], E, True, dtype)
    assert (y["pre"][code == 1] == 0).all() and (code == 1).any() and (y["pre"][(code == 2) | (code == 3)] != 0).all()
    ref_r = R.bn_bwd_reduce(s["dy"], None, s["x"], k["mean"], k["invstd"], k["scale"], k["shift"], E, True, nparts)
    ref_a = R.bn_bwd_apply(s["dy"], None, s["x"], k["mean"], k["invstd"], k["scale"], k["shift"], k["c1"], k["c2"], E, True, dtype)
    gref = on_dev(ref_r["gmask"], dtype)
    for form, dy, yy, relu in (("from y", s["dyd"], on_dev(y["y"], dtype), True), ("from x", s["dyd"], None, True),
                               ("pre-masked", gref, None, False)):
        part, gmask = nan(E, nparts, 2, C), nan(*s["x"].shape, dtype=dtype)
        dx, gm = nan(*s["x"].shape, dtype=dtype), nan(*s["x"].shape, dtype=dtype)
        ops.bn_bwd_reduce(dy, yy, s["xd"], kd["mean"], kd["invstd"], kd["scale"], kd["shift"], rpe, E, C, relu, part, nparts,
                          gmask=gmask)
        ops.bn_bwd_apply(dy, yy, s["xd"], kd["mean"], kd["invstd"], kd["scale"], kd["shift"], kd["c1"], kd["c2"], dx, gm, rpe, E, C,
                         relu)
        torch.cuda.synchronize()
        same(part, ref_r["part"], f"partial rows, mask {form}")
        same(gmask, ref_r["gmask"], f"gmask, mask {form}")
        same(gm, ref_a["gm"], f"gm, mask {form}")
        same(dx, ref_a["dx"], f"dx, mask {form}")


# ---------------------------------------------------------------------------------------------------------------------------------
# global-average-pool partial sums

@pytest.mark.parametrize("parts", R.NPARTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES + R.GAP_CASES, ids=ids(R.CASES + R.GAP_CASES))
def test_bn_apply_gap_matches_reference(case, kind, parts):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    k, kd = s["k"], s["kd"]
    nparts = R.nparts_of(parts, H * W)
    L = R.chain_stream(H * W, nparts, C, dtype)
    for relu in (True, False):
        ref = R.bn_apply_gap(s["x"], k["scale"], k["shift"], k["mean"], nparts, B, relu, dtype)
        y, part = nan(*s["x"].shape, dtype=dtype), nan(E * B, nparts, C)
        ops.bn_apply_gap(s["xd"], y, kd["scale"], kd["shift"], kd["mean"], part, nparts, B, relu)
        torch.cuda.synchronize()
        check_stored(y, ref["y"], ref["mag"], kind, dtype, f"bn_apply_gap y relu={relu}")
        # the sums are DEFINED over the stored y: in float32, where the stored y may differ from the reference's by its own bound,
        # they are held against the float64 sums of the y this launch stored (in bfloat16 that is the reference's y, bit for bit)
        psum, pabs = (ref["part"], ref["abs"]) if kind == "lattice" or dtype == BF16 else R.gap_sums(y.cpu().to(F64), nparts)
        check_sum(part, psum, pabs, L, kind, f"bn_apply_gap sums relu={relu}")


@pytest.mark.parametrize("b_form", ("none", "private", "shared"))
@pytest.mark.parametrize("parts", R.NPARTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.GAP_CASES, ids=ids(R.GAP_CASES))
def test_gap_partial_matches_reference(case, kind, parts, b_form):
    E, B, H, W, C, dtype = case
    s = setup(case, kind)
    nparts = R.nparts_of(parts, H * W)
    b, bd, ipe = {"none": (None, None, 0), "private": (s["dy"], s["dyd"], 0), "shared": (s["dy"][:B], s["dyd"][:B].contiguous(), B)}[b_form]
    ref = R.gap_partial(s["x"], b, nparts, ipe)
    part = nan(E * B, nparts, C)
    ops.gap_partial(s["xd"], bd, part, nparts, b_shared_ipe=ipe)
    torch.cuda.synchronize()
    check_sum(part, ref["part"], ref["abs"], R.chain_stream(H * W, nparts, C, dtype), kind, f"gap_partial b={b_form}")


# ---------------------------------------------------------------------------------------------------------------------------------
# reduce_partials and the finalize kernels: synthetic partial rows, no upstream kernel

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.REDUCE_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}")
def test_reduce_partials_matches_reference(shape, kind):
    nin, nout = shape
    E, width = 2, 2 * 136                       # 272 columns: more than one stride of the 256 threads, and not a multiple of it
    g = torch.Generator().manual_seed(nin + nout)
    if kind == "lattice":
        rows = torch.randint(-64, 65, (E, nin, width), generator=g).to(F64) / 4
    else:
        rows = (torch.randn(E, nin, width, generator=g) * (1 + torch.arange(nin)[None, :, None] / nin)).to(F32).to(F64)
    ref = R.reduce_partials(rows, nout)
    out = nan(E, nout, width)
    ops.reduce_partials(rows.to(F32).to(DEV), out, E, nin, nout, width)
    torch.cuda.synchronize()
    check_sum(out, ref["out"], ref["abs"], R.chain_reduce(nin, nout), kind, f"reduce_partials {nin} -> {nout}")


def table(tensors):
    """device array of per-expert pointers; None entries are null"""
    return torch.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch.int64, device=DEV)


def within(got, ref, bound, what):
    got = got.detach().cpu().to(F64)
    assert not torch.isnan(got).any(), f"{what}: unwritten elements"
    err = (got - ref).abs()
    print(f"{what}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", R.FIN_C)
@pytest.mark.parametrize("nparts", R.FIN_NPARTS)
def test_bn_finalize_matches_reference(nparts, C, kind):
    for E, count, with_shiftc, nulls in R.fin_configs(nparts, C):
        d = R.finalize_data(kind, E, nparts, C, count, 1000 * nparts + C + count)
        dev = lambda t: t.to(F32).to(DEV)
        partd = dev(d["part"])
        assert torch.equal(partd.cpu().to(F64), d["part"])
        on = torch.tensor([not (nulls and e == 1) for e in range(E)])
        gamma, beta = (None, None) if nulls else (d["gamma"], d["beta"])
        for training in (True, False):
            shiftc = d["shiftc"] if with_shiftc and training else None
            if not training:
                on = torch.ones(E, dtype=torch.bool)                       # eval mode reads every expert's running buffers
            ref = R.bn_finalize(d["part"], count, gamma, beta, (d["rmean"], d["rvar"], on), d["momentum"], d["eps"], training, shiftc)
            rm, rv = [dev(d["rmean"][e]) for e in range(E)], [dev(d["rvar"][e]) for e in range(E)]
            gd, bd = (None, None) if gamma is None else (dev(gamma), dev(beta))           # tables of rows of ONE live tensor
            tabs = [None if gd is None else table(list(gd)), None if bd is None else table(list(bd)),
                    table([rm[e] if on[e] else None for e in range(E)]), table([rv[e] if on[e] else None for e in range(E)])]
            scale, shift, mean, invstd = nan(E, C), nan(E, C), nan(E, C), nan(E, C)
            # eval mode must not read the partial rows at all: they are NaN there
            ops.bn_finalize(partd if training else nan(E, 1, 2, C), nparts if training else 0, count, tabs[0], tabs[1], tabs[2],
                            tabs[3], d["momentum"], d["eps"], training, scale, shift, mean, invstd, E, C, on_dev(shiftc, F32))
            torch.cuda.synchronize()
            what = f"bn_finalize E={E} count={count} shiftc={with_shiftc} nulls={nulls} training={training}"
            bound = R.finalize_bounds(ref, d, count, training, True)
            same(shift, ref["shift"], what + " shift")
            within(invstd, ref["invstd"], bound["invstd"], what + " invstd")
            within(scale, ref["scale"], bound["scale"], what + " scale")
            if kind == "lattice" or not training:
                same(mean, ref["mean"], what + " mean")
            else:
                within(mean, ref["mean"], bound["mean"], what + " mean")
            got_rm, got_rv = torch.stack(rm), torch.stack(rv)
            if not training:
                same(got_rm, d["rmean"], what + " running mean untouched")
                same(got_rv, d["rvar"], what + " running var untouched")
                continue
            off = ~on
            same(got_rm[off], d["rmean"][off], what + " running mean of a null entry")
            same(got_rv[off], d["rvar"][off], what + " running var of a null entry")
            if kind == "lattice":
                same(got_rm[on], ref["rmean"][on], what + " running mean")
            else:
                within(got_rm[on], ref["rmean"][on], bound["rmean"][on], what + " running mean")
            within(got_rv[on], ref["rvar"][on], bound["rvar"][on], what + " running var")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", R.FIN_C)
@pytest.mark.parametrize("nparts", R.FIN_NPARTS)
def test_bn_bwd_finalize_matches_reference(nparts, C, kind):
    for E, count, _, nulls in R.fin_configs(nparts, C):
        d = R.finalize_data(kind, E, nparts, C, count, 2000 * nparts + C + count)
        ref = R.bn_bwd_finalize(d["part"], count)
        dgamma, dbeta, c1, c2 = nan(E, C), nan(E, C), nan(E, C), nan(E, C)
        ops.bn_bwd_finalize(d["part"].to(F32).to(DEV), nparts, count, None if nulls else dgamma, None if nulls else dbeta, c1, c2, E, C)
        torch.cuda.synchronize()
        what = f"bn_bwd_finalize E={E} count={count} nulls={nulls}"
        outs = {"c1": (c1, ref["abs1"] / count), "c2": (c2, ref["abs2"] / count)}
        if nulls:
            assert torch.isnan(dgamma).all() and torch.isnan(dbeta).all()
        else:
            outs.update(dbeta=(dbeta, ref["abs1"]), dgamma=(dgamma, ref["abs2"]))
        for n, (got, rows_abs) in outs.items():
            if kind == "lattice":
                same(got, ref[n], f"{what} {n}")
            else:                                           # one rounding of the double fold's result, the fold itself below 2^-40
                within(got, ref[n], EPS * ref[n].abs() + 2.0 ** -40 * rows_abs, f"{what} {n}")


# ---------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch():
    E, B, H, W, C = 1, 2, 4, 4, 64
    lib = hip.load()
    N, rpe = E * B, B * H * W
    bf, BF, FP = torch.bfloat16, hip.DT_BF16, hip.DT_F32
    x = torch.zeros(N, H, W, C, dtype=bf, device=DEV)
    wide = torch.full((N, H, W, 3 * C), 7.0, dtype=bf, device=DEV)                  # a buffer every legal window fits in
    y, dx, gm = (torch.full((N, H, W, C), 7.0, dtype=bf, device=DEV) for _ in range(3))
    pooled = torch.full((N, H // 2, W // 2, C), 7.0, dtype=bf, device=DEV)
    y8 = torch.full((N, H, W, C), 7, dtype=torch.uint8, device=DEV)
    part, part2, shiftc = (torch.full((N, 4, 2, C), 7.0, device=DEV) for _ in range(3))
    k = [torch.ones(E, C, device=DEV) for _ in range(6)]
    tab = table([k[0][0]])
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def colstats(rows=rpe, e=E, c=C, ld=3 * C, coff=C, nparts=4, dtype=BF):
        return lib.pmoe_colstats(p(wide), rows, e, c, ld, coff, p(part), nparts, p(shiftc), dtype, None)

    def bwd_reduce(yy=y, scale=k[2], shift=k[3], c=C, nparts=4, dtype=BF, rows=rpe, e=E):
        return lib.pmoe_bn_bwd_reduce(p(x), p(yy), p(x), p(k[0]), p(k[1]), p(scale), p(shift), rows, e, c, 1, p(part), nparts, p(gm),
                                      dtype, None)

    def reduce(nin=4, nout=2, width=2 * C):
        return lib.pmoe_reduce_partials(p(part), p(part2), E, nin, nout, width, None)

    def finalize(training=0, rm=tab, rv=tab):
        return lib.pmoe_bn_finalize(p(part), 4, rpe, p(tab), p(tab), p(rm), p(rv), 0.1, 1e-5, training, p(k[2]), p(k[3]), p(k[4]),
                                    p(k[5]), E, C, None, None)

    def apply(c=C, ld=3 * C, coff=C, dtype=BF, f8=None):
        return lib.pmoe_bn_apply(p(x), None, p(wide), p(k[2]), p(k[3]), p(k[0]), rpe, E, c, 1, ld, coff, dtype, p(f8), 1.0, None)

    def pool2(xx=x, yy=wide, pp=pooled, ipe=B, h=H, w=W, e=E, c=C, ld=3 * C, coff=C, dtype=BF):
        return lib.pmoe_bn_apply_pool2(p(xx), p(yy), p(pp), p(k[2]), p(k[3]), p(k[0]), ipe, h, w, e, c, 1, ld, coff, dtype, None)

    def bwd_apply(c=C, dtype=BF):
        return lib.pmoe_bn_bwd_apply(p(x), p(y), p(x), p(k[0]), p(k[1]), p(k[2]), p(k[3]), p(k[4]), p(k[5]), p(dx), p(gm), rpe, E, c, 1,
                                     dtype, None)

    def gap(c=C, nparts=4, dtype=BF):
        return lib.pmoe_gap_partial(p(x), None, p(part), N, H * W, c, nparts, 0, dtype, None)

    def apply_gap(xx=x, yy=y, sc=k[2], sh=k[3], mu=k[0], pt=part, nparts=4, n=N, ipe=B, hw=H * W, c=C, dtype=BF):
        return lib.pmoe_bn_apply_gap(p(xx), p(yy), p(sc), p(sh), p(mu), p(pt), nparts, n, ipe, hw, c, 1, dtype, None)

    calls = {
        "C not a multiple of the vector width": [lambda: colstats(c=12), lambda: bwd_reduce(c=12), lambda: apply(c=12), lambda: pool2(c=12),
                                                 lambda: bwd_apply(c=12), lambda: gap(c=12), lambda: apply_gap(c=12),
                                                 lambda: colstats(c=6, dtype=FP), lambda: apply(c=6, dtype=FP), lambda: gap(c=6, dtype=FP)],
        "C / ve not a power of two": [lambda: colstats(c=24), lambda: bwd_reduce(c=24), lambda: apply(c=24), lambda: pool2(c=24),
                                      lambda: bwd_apply(c=24), lambda: colstats(c=12, dtype=FP), lambda: bwd_apply(c=12, dtype=FP)],
        "more than 256 channel vectors": [lambda: colstats(c=4096, ld=3 * 4096, coff=0), lambda: bwd_reduce(c=4096), lambda: apply(c=4096, ld=0),
                                          lambda: pool2(c=4096, ld=0), lambda: bwd_apply(c=4096), lambda: gap(c=4096),
                                          lambda: apply_gap(c=4096), lambda: gap(c=2048, dtype=FP)],
        "nparts < 1": [lambda: colstats(nparts=0), lambda: bwd_reduce(nparts=0), lambda: gap(nparts=0), lambda: apply_gap(nparts=-1)],
        "rows or experts < 1": [lambda: colstats(rows=0), lambda: colstats(e=0), lambda: bwd_reduce(rows=0), lambda: bwd_reduce(e=0),
                                lambda: pool2(ipe=0), lambda: pool2(e=0), lambda: apply_gap(n=0), lambda: apply_gap(ipe=0),
                                lambda: apply_gap(hw=0), lambda: apply_gap(n=3)],
        "window not on 16-byte vectors or outside the row": [
            lambda: colstats(ld=3 * C + 4), lambda: colstats(coff=4), lambda: colstats(coff=-8), lambda: colstats(coff=2 * C + 8),
            lambda: colstats(ld=C - 8, coff=0), lambda: colstats(ld=2, coff=0, c=4, dtype=FP),
            lambda: apply(ld=3 * C + 4), lambda: apply(coff=4), lambda: apply(coff=2 * C + 8),
            lambda: pool2(ld=3 * C + 4), lambda: pool2(coff=4), lambda: pool2(coff=2 * C + 8)],
        "recomputed mask without scale or shift": [lambda: bwd_reduce(yy=None, scale=None), lambda: bwd_reduce(yy=None, shift=None)],
        "empty reduction": [lambda: reduce(nin=0), lambda: reduce(nout=0), lambda: reduce(width=0)],
        "eval mode without running buffers": [lambda: finalize(rm=None), lambda: finalize(rv=None)],
        "fp8 side output of a float32 or windowed launch": [lambda: apply(f8=y8), lambda: apply(f8=y8, ld=0, dtype=FP)],
        "pool2 geometry or a null tensor": [lambda: pool2(h=3), lambda: pool2(w=5), lambda: pool2(h=0), lambda: pool2(w=1),
                                            lambda: pool2(xx=None), lambda: pool2(yy=None), lambda: pool2(pp=None)],
        "bn_apply_gap null tensor": [lambda: apply_gap(xx=None), lambda: apply_gap(yy=None), lambda: apply_gap(sc=None),
                                     lambda: apply_gap(sh=None), lambda: apply_gap(mu=None), lambda: apply_gap(pt=None)],
        "unknown dtype": [lambda: colstats(dtype=7), lambda: bwd_reduce(dtype=7), lambda: apply(dtype=7), lambda: pool2(dtype=7),
                          lambda: bwd_apply(dtype=7), lambda: gap(dtype=7), lambda: apply_gap(dtype=7)],
    }
    for what, fs in calls.items():
        for i, f in enumerate(fs):
            assert f() == hip.ERR_ARG, f"{what} (call {i})"
    torch.cuda.synchronize()
    for t in (wide, y, dx, gm, pooled, part, part2, shiftc):
        assert (t == 7.0).all(), "a refused call wrote to its outputs"
    assert (y8 == 7).all() and all((t == 1.0).all() for t in k)
    # the same buffers ARE valid: the well-formed calls succeed, the dense forms (ld <= 0) included
    assert colstats() == 0 and colstats(ld=0, coff=0) == 0 and colstats(ld=-1, coff=40) == 0
    assert bwd_reduce() == 0 and reduce() == 0 and finalize(training=1) == 0 and apply() == 0 and apply(ld=0, f8=y8) == 0
    assert pool2() == 0 and bwd_apply() == 0 and gap() == 0 and apply_gap() == 0
    torch.cuda.synchronize()
