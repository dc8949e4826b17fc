"""The pooling, ECA, layout, activation and mixture-head kernels of csrc/elementwise.hip and csrc/heads.hip, each against the
float64 reference of its own operation (tests/eca_head_ref.py), through pmoe_amd.ops.  Every kernel gets the REFERENCE's inputs,
never another kernel's output; outputs are NaN- or sentinel-filled before the launch and compared whole, pad channels, columns
outside a window and rows beyond the batch included; inputs must come back unmodified.

  lattice     small multiples of a power of two: float32 arithmetic is exact in any order (tests/test_eca_head_cpu.py proves it of
              every generator), every stored element equals the reference rounded once to the storage type
  continuous  randn-like data, redrawn where a float32 evaluation could land on the other side of a bfloat16 rounding boundary;
              bounds from float32 rounding and the measured error of the device's expf / expm1f / tanhf / logf (eca_head_ref)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests import eca_head_ref as R  # noqa: E402
from tests.test_bn_gpu import same  # noqa: E402

DEV = "cuda"
F64, F32, BF16 = R.F64, R.F32, R.BF16
EPS = R.EPS24
SENTINEL = -77.0
NAN = float("nan")


def ids(cases):
    return [R.case_id(c) for c in cases]


def dev(t, dtype=F32):
    """a reference tensor on the device in its storage type (which holds it exactly, NaN pads apart)"""
    if t is None:
        return None
    d = t.to(dtype).contiguous().to(DEV)
    assert torch.equal(torch.nan_to_num(d.cpu().to(F64), nan=12345.0), torch.nan_to_num(t, nan=12345.0)), "input not representable"
    return d


def filled(shape, dtype=F32, value=NAN):
    return torch.full(tuple(shape), value, dtype=dtype, device=DEV)


def unchanged(pairs):
    """inputs come back as they went in"""
    for name, (d, t) in pairs.items():
        if d is not None:
            got, ref = d.cpu().to(F64), t.to(F64)
            assert torch.equal(torch.nan_to_num(got, nan=12345.0), torch.nan_to_num(ref, nan=12345.0)), f"input {name} was modified"


def within(got, ref, bound, kind, what):
    """exact on the lattice, |got - ref| <= bound else; prints max err / bound"""
    got = got.detach().cpu().to(F64)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert not torch.isnan(got).any(), f"{what}: unwritten elements"
    if kind == "lattice":
        same(got, R.round_to(ref, F32), what)                  # (float32 outputs: the reference rounded once)
        return
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    print(f"{what}: max err / bound {ratio.max().item():.3f}")
    assert (err <= bound).all(), f"{what}: max err / bound {ratio.max().item():.3f}"


def stored(got, ref, mag, kind, dtype, what, extra=0.0, L=0):
    """a stored value: exact on the lattice and in bfloat16; float32: (L + 8) 2^-24 mag + half a unit in the last place + extra"""
    if kind == "lattice" or dtype == BF16:
        got = got.detach().cpu().to(F64)
        assert not torch.isnan(got).any(), f"{what}: unwritten elements"
        same(got, ref, what)
    else:
        within(got, ref, R.stored_bound(ref, mag, extra, L), kind, what)


def same_with_nan(got, ref, what):
    """whole-buffer comparison where the reference holds NaN for what must stay untouched (the buffer was NaN-filled)"""
    got = got.detach().cpu().to(F64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: written outside its rows or not written inside"
    same(torch.nan_to_num(got), torch.nan_to_num(ref), what)


def same_bits(got, ref, dtype, what):
    """bit for bit, the sign of a zero included"""
    r = ref.to(dtype)
    g = got.detach().cpu()
    it = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(g.view(it), r.view(it)), f"{what}: {(g.view(it) != r.view(it)).sum().item()} elements differ in bits"


def refused(fn, *a, **k):
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        fn(*a, **k)


def kinds_cases(cases, kinds_fn):
    return [pytest.param(c, k, id=f"{R.case_id(c)}-{k}") for c in cases for k in kinds_fn(c)]


# ---------------------------------------------------------------------------------------------------------------------------------
# max pool

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=ids(R.MAXPOOL_CASES))
def test_maxpool_fwd_bwd(case, kind):
    N, H, W, C, dtype = case
    d = R.maxpool_data(case, kind)
    ref = R.maxpool_fwd(d["x"])
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    xd, dyd = dev(d["x"], dtype), dev(d["dy"], dtype)
    y, am = filled((N, Ho, Wo, C), dtype), filled((N, Ho, Wo, C), torch.uint8, 255)
    ops.maxpool_fwd(xd, y, am)
    torch.cuda.synchronize()
    same(y, ref["y"], "maxpool y")
    assert torch.equal(am.cpu(), ref["am"]), f"argmax bytes: {(am.cpu() != ref['am']).sum().item()} differ"
    for name, amr in (("own", ref["am"]), ("any", d["am_any"])):
        amd = amr.to(DEV)
        dx = filled((N, H, W, C), dtype)
        ops.maxpool_bwd(dyd, amd, dx)
        torch.cuda.synchronize()
        assert not torch.isnan(dx).any()
        same(dx, R.maxpool_bwd(d["dy"], amr, H, W, dtype)["dx"], f"maxpool dx, {name} bytes")
        assert torch.equal(amd.cpu(), amr)
    unchanged({"x": (xd, d["x"]), "dy": (dyd, d["dy"])})


def test_maxpool_refusals():
    x = filled((1, 4, 4, 12), BF16, 0.0)
    refused(ops.maxpool_fwd, x, filled((1, 2, 2, 12), BF16), filled((1, 2, 2, 12), torch.uint8, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.GAP_PARTIAL_CASES, ids=ids(R.GAP_PARTIAL_CASES))
def test_gap_partial(case, kind):
    E, ipe, H, W, C, dtype, parts, form = case
    d = R.gap_partial_data(case, kind)
    nparts = R.nparts_of(parts, H * W)
    ref = R.gap_partial(d["a"], d["b"], nparts, d["b_ipe"])
    ad, bd = dev(d["a"], dtype), dev(d["b"], dtype)
    part = filled((E * ipe, nparts, C))
    ops.gap_partial(ad, bd, part, nparts, d["b_ipe"])
    torch.cuda.synchronize()
    L = R.chain_stream(H * W, nparts, C, dtype)
    within(part, ref["part"], (L + 8) * EPS * ref["part_abs"], kind, f"gap_partial {form} L {L}")
    unchanged({"a": (ad, d["a"]), "b": (bd, d["b"])})


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_gap_partial_refuses_more_than_256_channel_vectors(dtype):
    C = 257 * R.ve(dtype)
    refused(ops.gap_partial, filled((1, 1, 1, C), dtype, 0.0), None, filled((1, 1, C)), 1)


@pytest.mark.parametrize("case,kind", kinds_cases(R.GAP_FINISH_CASES, lambda c: R.kinds_of(c[3])))
def test_gap_finish(case, kind):
    N, C, nparts, HW, ld, coff, dtype = case
    d = R.gap_finish_data(case, kind)
    ref = R.gap_finish(d["part"], HW, dtype)
    pd = dev(d["part"])
    out = filled((N + 1, ld), dtype, SENTINEL)
    ops.gap_finish(pd, out, N, C, nparts, HW, ld, coff)
    torch.cuda.synchronize()
    stored(out[:N, coff:coff + C], ref["out"], ref["mag"], kind, dtype, "gap_finish", L=nparts)
    o = out.cpu().to(F64)
    o[:N, coff:coff + C] = SENTINEL
    assert (o == SENTINEL).all(), "gap_finish wrote outside its window"
    unchanged({"part": (pd, d["part"])})


@pytest.mark.parametrize("case,kind", kinds_cases(R.GAP_BWD_CASES, lambda c: R.kinds_of(c[1] * c[2])))
def test_gap_bwd(case, kind):
    N, H, W, C, ld, coff, dtype = case
    d = R.gap_bwd_data(case, kind)
    ref = R.gap_bwd(d["g"], H * W, C, coff, dtype)
    gd = dev(d["g"], dtype)
    dx = filled((N, H, W, C), dtype)
    ops.gap_bwd(gd, dx, ld, coff)
    torch.cuda.synchronize()
    exp = lambda t: t[:, None].expand(-1, H * W, -1).reshape(N, H, W, C)
    stored(dx, ref["dx"].reshape(N, H, W, C), exp(ref["mag"]), kind, dtype, "gap_bwd")
    unchanged({"g": (gd, d["g"])})


# ---------------------------------------------------------------------------------------------------------------------------------
# ECA

def w_table(w):
    rows = [dev(w[e].contiguous()) for e in range(w.shape[0])]
    return rows, hip.ptr_table(rows, DEV)


@pytest.mark.parametrize("case,kind", kinds_cases(R.ECA_CASES, lambda c: R.kinds_of(c[6])))
def test_eca_gate(case, kind):
    E, ipe, C, creal, k, nparts, HW, shared = case
    d = R.eca_data(case, kind)
    N = E * ipe
    ref = R.eca_gate(d["part"], HW, d["w"], k, N, ipe, ipe if shared else 0, C, creal)
    b = R.eca_gate_bounds(ref, nparts, k)
    pd = dev(d["part"])
    rows, tab = w_table(d["w"])
    gate, gapmean = filled((N + 1, C)), filled((N + 1, C))
    ops.eca_gate(pd, nparts, HW, tab, k, gate, gapmean, N, ipe, ipe if shared else 0, C, creal)
    torch.cuda.synchronize()
    within(gapmean[:N], ref["gapmean"], b["gapmean"], kind, "eca gapmean")
    within(gate[:N], ref["gate"], b["gate"], kind, "eca gate")
    if creal < C:                                                    # +0 in the pad channels, exactly
        assert (gate[:N, creal:] == 0).all() and (gapmean[:N, creal:] == 0).all()
    assert torch.isnan(gate[N]).all() and torch.isnan(gapmean[N]).all(), "a row beyond N was written"
    unchanged({"part": (pd, d["part"]), "w": (torch.stack(rows), d["w"])})


@pytest.mark.parametrize("form", R.DGAP_FORMS)
@pytest.mark.parametrize("case,kind", kinds_cases(R.ECA_CASES, lambda c: R.kinds_of(c[6])))
def test_eca_bwd_small(case, kind, form):
    E, ipe, C, creal, k, nparts, HW, shared = case
    d = R.eca_data(case, kind)
    N = E * ipe
    scale = 1.0 / HW if form == "1/HW" else 1.0
    ref = R.eca_bwd_small(d["dot_part"], d["gate_in"], d["gapmean_in"], d["w_b"], k, ipe, C, creal, scale)
    b = R.eca_bwd_small_bounds(ref, nparts, k, ipe, C)
    ins = {n: (dev(d[n]), d[n]) for n in ("dot_part", "gate_in", "gapmean_in")}
    rows, tab = w_table(d["w_b"])
    dgap = None if form == "null" else filled((N + 1, C))
    dw = filled((E + 1, k))
    ops.eca_bwd_small(ins["dot_part"][0], nparts, ins["gate_in"][0], ins["gapmean_in"][0], tab, k, dgap, dw, N, ipe, C, creal, scale)
    torch.cuda.synchronize()
    within(dw[:E], ref["dw"], b["dw"], kind, f"eca dw L {b['L']}")
    assert torch.isnan(dw[E]).all()
    if dgap is not None:
        within(dgap[:N], ref["dgap"], b["dgap"] + EPS * ref["dgap"].abs(), kind, "eca dgap")
        assert (dgap[:N, creal:] == 0).all() and torch.isnan(dgap[N]).all()
    ins["w"] = (torch.stack(rows), d["w_b"])
    unchanged(ins)


def test_eca_refusals():
    """C > 1024, k > 9 and an even k: refused by the gate and by its backward alike"""
    z = lambda *s: filled(s, F32, 0.0)
    _, tab = w_table(torch.zeros(1, 12, dtype=F64))
    for C, k in ((1025, 3), (64, 11), (64, 4), (64, 2), (64, 0)):
        refused(ops.eca_gate, z(1, 1, C), 1, 4, tab, k, z(1, C), z(1, C), 1, 1, 0, C, C)
        refused(ops.eca_bwd_small, z(1, 1, C), 1, z(1, C), z(1, C), tab, k, z(1, C), z(1, 12), 1, 1, C, C)
    refused(ops.eca_bwd_small, z(3, 1, 64), 1, z(3, 64), z(3, 64), tab, 3, z(3, 64), z(1, 3), 3, 2, 64, 64)      # N % ipe


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.ECA_SCALE_CASES, ids=ids(R.ECA_SCALE_CASES))
def test_eca_scale(case, kind):
    E, ipe, H, W, C, shared, dtype = case
    d = R.eca_scale_data(case, kind)
    ref = R.eca_scale(d["x"], d["gate"], ipe if shared else 0, dtype)
    xd, gd = dev(d["x"], dtype), dev(d["gate"])
    y = filled((E * ipe, H, W, C), dtype)
    ops.eca_scale(xd, gd, y, ipe if shared else 0)
    torch.cuda.synchronize()
    stored(y, ref["y"], ref["mag"], kind, dtype, "eca_scale")
    unchanged({"x": (xd, d["x"]), "gate": (gd, d["gate"])})


@pytest.mark.parametrize("case,kind", kinds_cases(R.ECA_APPLY_CASES, lambda c: R.kinds_of(c[1] * c[2])))
def test_eca_bwd_apply(case, kind):
    N, H, W, C, dtype = case
    d = R.eca_apply_data(case, kind)
    ref = R.eca_bwd_apply(d["dy"], d["gate"], d["dgap"], dtype)
    dyd, gd, dgd = dev(d["dy"], dtype), dev(d["gate"]), dev(d["dgap"])
    dx = filled((N, H, W, C), dtype)
    ops.eca_bwd_apply(dyd, gd, dgd, dx)
    torch.cuda.synchronize()
    stored(dx, ref["dx"], ref["mag"], kind, dtype, "eca_bwd_apply")
    unchanged({"dy": (dyd, d["dy"]), "gate": (gd, d["gate"]), "dgap": (dgd, d["dgap"])})


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.STEM_FOLD_CASES, ids=ids(R.STEM_FOLD_CASES))
def test_eca_stem_fold(case, kind):
    E, ipe, cout, coutp, cin, gld, cinp, ks = case
    d = R.stem_fold_data(case, kind)
    N, taps = E * ipe, ks * ks
    ref = R.eca_stem_fold(d["G"], d["gate"], d["w"], ipe, cout, cin, taps)
    Ldw, Lds = R.stem_fold_chains(ipe, cout, taps, gld)
    Gd, gd = dev(d["G"]), dev(d["gate"])
    rows, tab = w_table(d["w"].reshape(E, -1))
    dw, ds = filled((E + 1, cout, cin, taps)), filled((N + 1, gld))
    ops.eca_stem_fold(Gd, gd, tab, dw, ds, N, ipe, cout, cin, ks, coutp, cinp)
    torch.cuda.synchronize()
    within(dw[:E], ref["dw"], (Ldw + 8) * EPS * ref["dw_abs"], kind, f"stem fold dw L {Ldw}")
    within(ds[:N], ref["ds"], (Lds + 8) * EPS * ref["ds_abs"], kind, f"stem fold ds L {Lds}")
    assert (ds[:N, cin:] == 0).all() and torch.isnan(ds[N]).all() and torch.isnan(dw[E]).all()
    unchanged({"G": (Gd, d["G"]), "gate": (gd, d["gate"]), "w": (torch.stack(rows), d["w"].reshape(E, -1))})


def test_eca_stem_fold_refuses_rows_over_256():
    z = lambda *s: filled(s, F32, 0.0)
    _, tab = w_table(torch.zeros(1, 5 * 12, dtype=F64))
    refused(ops.eca_stem_fold, z(1, 1, 64, 272), z(1, 272), tab, z(1, 5, 12, 1), z(1, 272), 1, 1, 5, 12, 1, 64, 272)


def test_pack_bias():
    for E, cout, coutp in R.PACK_BIAS_CASES:
        src = R.latw(R.gen("pack_bias", E, cout), (E, cout), F32)
        rows, tab = w_table(src)
        dst = filled((E + 1, coutp))
        ops.pack_bias(tab, dst, E, cout, coutp)
        torch.cuda.synchronize()
        same_bits(dst[:E], R.pack_bias(src, coutp)["dst"], F32, f"pack_bias {E}x{cout}->{coutp}")
        assert torch.isnan(dst[E]).all()
        unchanged({"src": (torch.stack(rows), src)})


# ---------------------------------------------------------------------------------------------------------------------------------
# layout

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.NHWC_CASES, ids=ids(R.NHWC_CASES))
def test_nchw_to_nhwc(case, kind):
    B, C, H, W, Cp, dtype = case
    d = R.nhwc_data(case, kind)
    sd = d["src"].to(F32).to(DEV)
    dst = filled((B + 1, H, W, Cp), dtype)
    ops.nchw_to_nhwc(sd, dst[:B])
    torch.cuda.synchronize()
    same_bits(dst[:B], R.nchw_to_nhwc(d["src"], Cp, dtype)["dst"], dtype, f"nchw_to_nhwc {R.nhwc_route(B, C, H, W, Cp)}")
    assert torch.isnan(dst[B]).all(), "an image beyond B was written"
    same_bits(sd, d["src"], F32, "src")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.PAD_ROWS_CASES, ids=ids(R.PAD_ROWS_CASES))
def test_pad_rows(case, kind):
    B, K, Kp, dtype = case
    g = R.gen("pad_rows", case, kind)
    src = R.latw(g, (B, K), F32) if kind == "lattice" else R.randn(g, (B, K))
    src[0, 0] = -0.0
    sd = src.to(F32).to(DEV)
    dst = filled((B + 1, Kp), dtype)
    ops.pad_rows(sd, dst[:B])
    torch.cuda.synchronize()
    same_bits(dst[:B], R.pad_rows(src, Kp, dtype)["dst"], dtype, "pad_rows")
    assert torch.isnan(dst[B]).all()
    same_bits(sd, src, F32, "src")


# ---------------------------------------------------------------------------------------------------------------------------------
# activation + dropout

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.ACT_CASES, ids=ids(R.ACT_CASES))
def test_act_fwd_bwd(case, kind):
    n, act, p, seed, dtype = case
    d = R.act_data(case, kind)
    ref = R.act_fwd(d["x"], act, p, seed, dtype)
    xd = dev(d["x"], dtype)
    y = filled((n + R.ve(dtype),), dtype)
    ops.act_fwd(xd, y[:n], act, p, seed)
    torch.cuda.synchronize()
    if p > 0:
        # the dropout mask, element for element, wherever act(x) != 0 lets the output show it
        seen = R.act_apply(act, d["x"]) != 0
        assert torch.equal((y[:n].cpu().to(F64) != 0)[seen], ref["keep"][seen]), "dropout mask differs from the hash mask"
        assert 0.4 < ref["keep"].to(F64).mean().item() < 0.6 or n < 64
    stored(y[:n], ref["y"], ref["mag"], kind, dtype, f"act_fwd act {act} p {p}", extra=ref["allow"])
    assert torch.isnan(y[n:]).all(), "act_fwd wrote past n"
    yd, dyd = dev(d["y"], dtype), dev(d["dy"], dtype)
    rb = R.act_bwd(d["dy"], d["y"], act, p, dtype)
    dx = filled((n + R.ve(dtype),), dtype)
    ops.act_bwd(dyd, yd, dx[:n], act, p)
    torch.cuda.synchronize()
    stored(dx[:n], rb["dx"], rb["mag"], kind, dtype, f"act_bwd act {act} p {p}")
    assert torch.isnan(dx[n:]).all(), "act_bwd wrote past n"
    unchanged({"x": (xd, d["x"]), "y": (yd, d["y"]), "dy": (dyd, d["dy"])})


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_act_refuses_a_partial_vector(dtype):
    n = R.ve(dtype) + 1
    x = filled((n,), dtype, 0.0)
    refused(ops.act_fwd, x, filled((n,), dtype), R.ACT_RELU)
    refused(ops.act_bwd, x, x, filled((n,), dtype), R.ACT_RELU)


# ---------------------------------------------------------------------------------------------------------------------------------
# mixture head

@pytest.mark.parametrize("case,kind", kinds_cases(R.GATE_CASES, R.gate_kinds))
def test_gate_mixture_fwd(case, kind):
    E, B, ar, shared, dtype = case
    d = R.gate_data(case, kind)
    ref = R.gate_fwd(d["head"], d["spd"], B, E, ar, shared)
    hd, sd = dev(d["head"], dtype), dev(d["spd"], dtype)
    probs, mean, std = filled((B + 1, E)), filled((B + 1, E, 2)), filled((B + 1, E, 2))
    speeds = filled((B + 1, 1) if shared else (B + 1, E, 1))
    ops.gate_mixture_fwd(hd, sd, probs, mean, std, speeds, B, E, ar, shared)
    torch.cuda.synchronize()
    within(probs[:B], ref["probs"], ref["probs_bound"], kind, f"gate probs G {R.gate_G(E)}")
    within(std[:B], ref["std"], ref["std_bound"], kind, "gate std")
    same(mean[:B], ref["mean"], "gate mean")
    same(speeds[:B], ref["speeds"], "gate speeds")
    for t in (probs, mean, std, speeds):
        assert torch.isnan(t[B]).all(), "a row beyond B was written"
    unchanged({"head": (hd, d["head"]), "spd": (sd, d["spd"])})


@pytest.mark.parametrize("case,kind", kinds_cases(R.GATE_CASES, lambda c: R.KINDS))
def test_gate_mixture_bwd(case, kind):
    """every gradient given, then each of them null in turn"""
    for null in R.GATE_NULLS:
        _gate_bwd(case, kind, null)


def _gate_bwd(case, kind, null):
    E, B, ar, shared, dtype = case
    d = R.gate_data(case, kind)
    g = {n: (None if n == null else d[n]) for n in ("dprobs", "dmean", "dstd", "dspeeds")}
    rows, ld = d["rows"], d["ld"]
    ref = R.gate_bwd(d["head"], d["probs"], g["dprobs"], g["dmean"], g["dstd"], g["dspeeds"], B, E, ar, shared, rows, ld, R.SPD_LD, dtype)
    hd, pd = dev(d["head"], dtype), dev(d["probs"])
    gd = {n: dev(t) for n, t in g.items()}
    dhead, dspd = filled((rows, ld), dtype), filled((rows, R.SPD_LD), dtype)
    ops.gate_mixture_bwd(hd, pd, gd["dprobs"], gd["dmean"], gd["dstd"], gd["dspeeds"], dhead, dspd, B, E, ar, shared)
    torch.cuda.synchronize()
    same_with_nan(dspd, ref["dspd"], f"dspd (null {null})")                     # column 0 rounded once, the rest zero, two rows untouched
    got = dhead.cpu().to(F64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref["dhead"])), "dhead: rows beyond the layout written, or elements left unwritten"
    G = R.gate_G(E)
    stored(torch.nan_to_num(dhead), torch.nan_to_num(ref["dhead"]), ref["mag"], kind, dtype, f"dhead (null {null}) G {G}",
           extra=ref["allow"], L=int(math.log2(G)))
    unchanged({"head": (hd, d["head"]), "probs": (pd, d["probs"]), **{n: (gd[n], g[n]) for n in g}})


def test_gate_mixture_refusals():
    z = lambda *s: filled(s, F32, 0.0)
    for shared, E in ((False, 4), (True, 4)):
        ld = (5 * E if shared else 5) - 1                                       # one below the minimum
        rows = 2 if shared else 2 * E
        refused(ops.gate_mixture_fwd, z(rows, ld), z(rows, 4), z(2, E), z(2, E, 2), z(2, E, 2), z(2, E, 1), 2, E, 0, shared)
        refused(ops.gate_mixture_bwd, z(rows, ld), z(2, E), z(2, E), z(2, E, 2), z(2, E, 2), z(2, E, 1), z(rows, ld), z(rows, 4),
                2, E, 0, shared)
    refused(ops.gate_mixture_fwd, z(65, 8), z(65, 4), z(1, 65), z(1, 65, 2), z(1, 65, 2), z(1, 65, 1), 1, 65, 0, False)
    refused(ops.moe_loss, z(1, 65), z(1, 65, 2), z(1, 65, 2), z(1, 65, 1), z(1, 2), z(1), 0.5, 0.5, z(1), z(1), z(1, 65), z(1, 65, 2),
            z(1, 65, 2), z(1, 65, 1), 1, 65)


@pytest.mark.parametrize("case,kind", kinds_cases(R.LOSS_CASES, R.loss_kinds))
def test_moe_loss(case, kind):
    E, B, shared = case
    d = R.loss_data(case, kind)
    c0, c1 = d["c"]
    args = [d[n] for n in ("probs", "mean", "std", "speeds", "act", "tgt")]
    ref = R.moe_loss(*args, c0, c1, B, E, shared)
    dv = [dev(t) for t in args]
    out = {"loss": filled((2,)), "loglik": filled((B + 1,)), "dprobs": filled((B + 1, E)), "dmean": filled((B + 1, E, 2)),
           "dstd": filled((B + 1, E, 2)), "dspeeds": filled((B + 1, 1) if shared else (B + 1, E, 1))}
    ops.moe_loss(*dv, c0, c1, out["loss"], out["loglik"], out["dprobs"], out["dmean"], out["dstd"], out["dspeeds"], B, E, shared)
    torch.cuda.synchronize()
    nrows = {n: (1 if n == "loss" else B) for n in out}
    if kind == "lattice":                                            # c0 = 0: the speed branch alone is exact
        same(out["loss"][:1], ref["loss"], "loss (mse term)")
        same(out["dspeeds"][:B], ref["dspeeds"], "dspeeds")
        for n in ("dprobs", "dmean", "dstd"):
            same(out[n][:B], torch.zeros_like(ref[n]), n)
    else:
        bounds = R.moe_loss_bounds(ref, *args, c0, c1, B, E, shared)
        for n in out:
            within(out[n][:nrows[n]], ref[n], bounds[n], kind, f"moe_loss {n}")
        if E > 1:
            assert ref["clamped"][0, E - 1] and out["dprobs"][0, E - 1].item() == 0, "the clamped probability has a gradient"
    for n, t in out.items():
        assert torch.isnan(t[nrows[n]:]).all(), f"{n}: written beyond its rows"
    unchanged({n: (dv[i], args[i]) for i, n in enumerate(("probs", "mean", "std", "speeds", "act", "tgt"))})


# ---------------------------------------------------------------------------------------------------------------------------------
# the device library's transcendental functions, as measured for the T_f constants of tests/eca_head_ref.py

def test_device_library_error_is_within_the_constants():
    """dense sweeps through the entry points themselves; prints the worst error per function in units in the last place"""
    n = 1 << 20
    ulp = lambda v: torch.ldexp(torch.ones_like(v), torch.frexp(v.abs().clamp_min(1e-300))[1] - 24)      # of the float32 nearest v
    worst = {}

    def sweep_act(act, lo, hi):
        x = (torch.rand(n, generator=R.gen("tf", act), dtype=F64) * (hi - lo) + lo).to(F32)
        y = filled((n,))
        ops.act_fwd(x.to(DEV), y, act)
        torch.cuda.synchronize()
        return x.to(F64), y.cpu().to(F64)

    x, y = sweep_act(R.ACT_ELU, -16.0, -2.0 ** -20)
    worst["expm1"] = ((y - torch.expm1(x)).abs() / ulp(torch.expm1(x))).max().item()
    x, y = sweep_act(R.ACT_TANH, -9.0, 9.0)
    worst["tanh"] = ((y - torch.tanh(x)).abs() / ulp(torch.tanh(x))).max().item()
    x, y = sweep_act(R.ACT_SIGMOID, -16.0, 0.0)
    s = torch.sigmoid(x)
    worst["exp (sigmoid)"] = ((y - s).abs() / (R.ULP * s * (1 - s))).max().item()
    # expf(r), r <= 0, through gate_mixture_bwd in the shared layout with E = 1: dhead[:, 2] = dstd * expf(raw)
    B = 1 << 16
    head = torch.zeros(B, 8, dtype=F64)
    head[:, 2] = -(torch.rand(B, generator=R.gen("tf", "exp"), dtype=F64) * 16).to(F32).to(F64)
    dstd = torch.ones(B, 1, 2, dtype=F64)
    dhead, dspd = filled((B, 8)), filled((B, 4))
    ops.gate_mixture_bwd(dev(head), dev(torch.ones(B, 1, dtype=F64)), None, None, dev(dstd), None, dhead, dspd, B, 1, 0, True)
    torch.cuda.synchronize()
    e = torch.exp(head[:, 2])
    worst["exp"] = ((dhead[:, 2].cpu().to(F64) - e).abs() / ulp(e)).max().item()
    # logf through moe_loss at E = 1, a = mu (z = 0), sigma_1 = 1: ll = -logf(sigma_0) - 2 * log(2 pi) / 2
    B = 1 << 12
    lo, hi = math.log(2.0 ** -6), -2.0
    sg = torch.ones(B, 1, 2, dtype=F64)
    sg[:, 0, 0] = torch.exp(torch.rand(B, generator=R.gen("tf", "log"), dtype=F64) * (hi - lo) + lo).to(F32).to(F64)
    zeros = torch.zeros(B, 1, 2, dtype=F64)
    ll = filled((B,))
    ops.moe_loss(dev(torch.ones(B, 1, dtype=F64)), dev(zeros), dev(sg), dev(torch.zeros(B, 1, 1, dtype=F64)), dev(torch.zeros(B, 2, dtype=F64)),
                 dev(torch.zeros(B, dtype=F64)), 1.0, 0.0, filled((1,)), ll, filled((B, 1)), filled((B, 1, 2)), filled((B, 1, 2)),
                 filled((B, 1, 1)), B, 1)
    torch.cuda.synchronize()
    lg = torch.log(sg[:, 0, 0])
    worst["log"] = ((ll.cpu().to(F64) - (-lg - 2 * R.HALF_LOG_2PI)).abs() / ulp(lg)).max().item()
    print("measured worst error, units in the last place:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["expm1"] <= R.T_EXPM1 and worst["tanh"] <= R.T_TANH and worst["log"] <= R.T_LOG
    assert max(worst["exp"], worst["exp (sigmoid)"]) <= R.T_EXP
