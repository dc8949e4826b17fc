"""The reference of the U-Net, segmentation-loss and action-head kernels (tests/unet_ref.py) proven on the CPU, before any GPU run:
it equals torch and the oracle in float64; its lattice generators are exact in float32 in two summation orders; the float32 CPU
evaluation of every continuous case lies inside the bound the GPU test uses; every case that claims a route takes it; every mutant
is caught on some case; and the library refuses what this revision newly refuses."""
import pytest
import torch
import torch.nn.functional as Fn

from oracle import pmoe_oracle as O
from pmoe_amd import hip
from tests import entry_refusals as ER
from tests import unet_ref as R
from tests.stage0_util import dice_oracle

F64, F32, BF16 = R.F64, R.F32, R.BF16
NANV = 12345.0


def eq(a, b):
    """equal, NaN matching NaN"""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a.to(F64), nan=NANV), torch.nan_to_num(b.to(F64), nan=NANV))


def close(a, b, rel=1e-12):
    a, b = a.to(F64), b.to(F64)
    return a.shape == b.shape and bool(((a - b).abs() <= rel * b.abs().clamp_min(1e-300) + 1e-300).all())


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference equals torch / the oracle in float64

@pytest.mark.parametrize("case", R.POOL_CASES, ids=[R.case_id(c) for c in R.POOL_CASES])
def test_pool_reference_is_torch_max_pool2d_and_its_autograd(case):
    d = R.pool_data(case)
    C, co = d["C"], d["x_coff"]
    v = nchw(d["x"][..., co:co + C]).requires_grad_(True)
    y = Fn.max_pool2d(v, 2, 2)
    assert eq(nhwc(y.detach()), R.maxpool2s2_fwd(d["x"], C, co)["y"])
    N, H, W = d["x"].shape[:3]
    if H * W >= 35:          # every planted window: two NaNs, one NaN, all -inf
        assert torch.isnan(y).any() and torch.isinf(y).any()
    if H % 2 or W % 2:
        return
    y.backward(nchw(d["dy"]))
    want = nhwc(v.grad)
    if d["dskip"] is not None:
        want = want + d["dskip"][..., d["ds_coff"]:d["ds_coff"] + C]
    got = R.maxpool2s2_bwd(d["x"], d["dy"], d["dskip"], C, co, d["ds_coff"], F64)["dx"]
    assert eq(got, want)
    for dt in R.DTYPES:        # the sums are exact in either storage type
        assert eq(R.maxpool2s2_bwd(d["x"], d["dy"], d["dskip"], C, co, d["ds_coff"], dt)["dx"], want)


def shuffle_src(case):
    N, H, W, cv, extra, dmul, doff, dtype = case
    C = cv * R.ve(dtype)
    src = R.nanlike((N, H, W, 4 * C + extra * R.ve(dtype)))
    src[..., :4 * C] = R.lat(R.gen("shuffle", case), (N, H, W, 4 * C), 64, 4)
    return src, C, dmul * C, doff * C


@pytest.mark.parametrize("case", R.SHUFFLE_CASES, ids=[R.case_id(c) for c in R.SHUFFLE_CASES])
def test_shuffle_reference_is_torch_pixel_shuffle_and_the_pair_are_inverses(case):
    src, C, dld, dco = shuffle_src(case)
    N, H, W, _ = src.shape
    dst = R.pixel_shuffle2(src, C, dld, dco)["dst"]
    t = src[..., :4 * C].reshape(N, H, W, 4, C).permute(0, 4, 3, 1, 2).reshape(N, 4 * C, H, W)
    assert eq(dst[..., dco:dco + C], nhwc(Fn.pixel_shuffle(t, 2)))
    outside = dst.clone()
    outside[..., dco:dco + C] = R.NAN
    assert torch.isnan(outside).all()
    back = R.pixel_unshuffle2(dst, C, dco, src.shape[-1])["dst"]
    assert eq(back, src)
    u = nhwc(Fn.pixel_unshuffle(nchw(dst[..., dco:dco + C]), 2)).reshape(N, H, W, C, 4).permute(0, 1, 2, 4, 3).reshape(N, H, W, 4 * C)
    assert eq(back[..., :4 * C], u)


@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=[R.case_id(c) for c in R.WINDOW_CASES])
def test_window_reference_and_its_bfloat16_sums(case):
    rows, C, sld, sco, dld, dco, dtype = case
    d = R.window_data(case)
    cp = R.copy_window(d["src"], sco, dld, dco, C)["dst"]
    assert eq(cp[:, dco:dco + C], d["src"][:, sco:sco + C]) and torch.isnan(cp).sum() == rows * (dld - C)
    ad = R.add_window(d["src"], sco, d["dst"], dco, C, dtype)
    assert eq(ad["dst"][:, dco:dco + C], (d["src"][:, sco:sco + C] + d["dst"][:, dco:dco + C]).to(F32).to(dtype).to(F64))
    assert torch.isnan(ad["dst"]).sum() == rows * (dld - C)
    # no sum near a rounding boundary: rounding the float32 sum or the exact one gives the same value
    s32 = (d["src"][:, sco:sco + C].to(F32) + d["dst"][:, dco:dco + C].to(F32)).to(dtype).to(F64)
    assert eq(s32, ad["dst"][:, dco:dco + C])
    assert not R.near_boundary(ad["raw"], R.TOL * ad["raw"].abs(), dtype).any()


@pytest.mark.parametrize("case", R.CAT_CASES, ids=[R.case_id(c) for c in R.CAT_CASES])
def test_cat_reference_is_torch_cat(case):
    K, c, sld, sco, dst_c, dst_ld, rows, dtype = case
    srcs = R.cat_data(case)["srcs"]
    dst = R.cat_windows(srcs, c, sco, dst_ld, dst_c)["dst"]
    want = torch.cat([s[:, sco:sco + c] for s in srcs] + [torch.zeros(rows, dst_c - K * c, dtype=F64),
                                                         R.nanlike((rows, dst_ld - dst_c))], 1)
    assert eq(dst, want) and not torch.isnan(dst[:, :dst_c]).any()


def test_nchw_reference_is_a_permute():
    for case in R.NCHW_CASES:
        N, HW, C, ld, coff, dtype = case
        src = R.nchw_data(case)["src"]
        dst = R.nhwc_to_nchw(src, C, coff)["dst"]
        assert eq(dst, nchw(src[..., coff:coff + C])) and not torch.isnan(dst).any()
        assert torch.isnan(src).sum() == N * HW * (ld - C)


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=[R.case_id(c) for c in R.HEAD_CASES])
@pytest.mark.parametrize("kind", R.KINDS)
def test_action_head_reference(case, kind):
    B, hld, sld, dtype = case
    d = R.head_data(case, kind)
    f = R.action_head_fwd(d["head"], d["spd"], B)
    assert eq(f["actions"], torch.tanh(d["head"][:B, :2])) and eq(f["speeds"], d["spd"][:B, 0])
    z = d["head"][:B, :2].clone().requires_grad_(True)
    torch.tanh(z).backward(d["dact"])
    a64 = torch.tanh(d["head"][:B, :2])
    r = R.action_head_bwd(a64, d["dact"], d["dspeeds"], d["rows"], hld, sld, B, F64)
    assert ((r["dhead"][:B, :2] - z.grad).abs() <= 1e-12 * r["mag"]).all() and eq(r["dspd"][:B, 0], d["dspeeds"])
    assert (r["dhead"][:B, 2:] == 0).all() and (r["dspd"][:B, 1:] == 0).all()
    assert torch.isnan(r["dhead"][B:]).all() and torch.isnan(r["dspd"][B:]).all()
    for null in ("dact", "dspeeds"):
        rn = R.action_head_bwd(d["actions"], None if null == "dact" else d["dact"], None if null == "dspeeds" else d["dspeeds"],
                               d["rows"], hld, sld, B, dtype)
        assert (rn["dhead" if null == "dact" else "dspd"][:B] == 0).all()
    r = R.action_head_bwd(d["actions"], d["dact"], d["dspeeds"], d["rows"], hld, sld, B, dtype)
    a32, g32 = d["actions"].to(F32), d["dact"].to(F32)
    raw32 = (g32 * (1 - a32 * a32)).to(F64)
    if kind == "lattice":
        assert eq(f["actions"].to(F32).to(F64), d["actions"]) and set(d["actions"].flatten().tolist()) <= {0.0, 1.0, -1.0}
        assert eq(raw32, r["raw"]) and eq(R.round_to(raw32, dtype), r["dhead"][:B, :2])
    else:
        assert (d["head"][:B].abs() <= 9).all()
        if dtype == BF16:
            assert eq(R.round_to(raw32, dtype), r["dhead"][:B, :2])
        else:
            assert ((raw32 - r["raw"]).abs() <= R.stored_bound(r["raw"], r["mag"])).all()
        fb = R.action_head_fwd_bounds(f)["actions"]
        assert ((torch.tanh(d["head"][:B, :2].to(F32)).to(F64) - f["actions"]).abs() <= fb).all()


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=[R.case_id(c) for c in R.LOSS_CASES])
@pytest.mark.parametrize("kind", R.KINDS)
def test_action_loss_reference(case, kind):
    B, ws = case
    d = R.loss_data(case, kind)
    c0, c1 = R.LOSS_C
    r = R.action_loss(d["actions"], d["speeds"], d["gt"], d["spd_gt"], c0, c1, B)
    a = d["actions"].clone().requires_grad_(True)
    loss = c0 * Fn.l1_loss(a, d["gt"])
    if ws:
        s = d["speeds"].clone().requires_grad_(True)
        loss = loss + c1 * Fn.mse_loss(s, d["spd_gt"])
    loss.backward()
    assert close(r["loss"], loss.detach()) and close(r["dact"], a.grad)
    assert (d["actions"] == d["gt"]).any() and (r["dact"][d["actions"] == d["gt"]] == 0).all()
    if ws:
        assert close(r["dspeeds"], s.grad)
    else:
        assert r["dspeeds"] is None
    b = R.action_loss_bounds(r, c0, c1, B, kind)
    f32 = lambda t: None if t is None else t.to(F32)       # noqa: E731
    for flip in (False, True):
        o = (lambda t: None if t is None else t.flip(0)) if flip else (lambda t: t)
        r32 = R.action_loss(o(f32(d["actions"])), o(f32(d["speeds"])), o(f32(d["gt"])), o(f32(d["spd_gt"])), c0, c1, B)
        if kind == "lattice":
            assert r32["l1"].to(F64) == r["l1"] and r32["l2"].to(F64) == r["l2"]
        assert (r32["loss"].to(F64) - r["loss"]).abs() <= b["loss"]
        assert ((o(r["dact"]) - r32["dact"].to(F64)).abs() <= o(b["dact"])).all()
        if ws:
            assert ((o(r["dspeeds"]) - r32["dspeeds"].to(F64)).abs() <= o(b["dspeeds"])).all()


@pytest.mark.parametrize("B", R.BLEND_CASES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_blend_reference_is_linear_tanh_and_its_autograd(B, kind):
    d = R.blend_data(B, kind)
    w = {k: d[k].clone().requires_grad_(True) for k in ("lat_w", "lat_b", "long_w", "long_b")}
    pu = d["pu"].clone().requires_grad_(True)
    lat = Fn.linear(torch.stack([d["moe"][:, 0], pu[:, 0]], -1), w["lat_w"][None], w["lat_b"])
    lon = Fn.linear(torch.stack([d["moe"][:, 1], pu[:, 1]], -1), w["long_w"][None], w["long_b"])
    out = torch.tanh(torch.cat([lat, lon], -1))
    f = R.blend_fwd(d["moe"], d["pu"], d["lat_w"], d["lat_b"], d["long_w"], d["long_b"])
    assert close(f["out"], out.detach())
    out.backward(d["dout"])
    r = R.blend_bwd(d["moe"], d["pu"], d["lat_w"], d["long_w"], out.detach(), d["dout"])
    auto = torch.stack([torch.cat([w["lat_w"].grad, w["lat_b"].grad]), torch.cat([w["long_w"].grad, w["long_b"].grad])])
    assert ((r["sums"] - auto).abs() <= 1e-12 * r["sums_abs"]).all()
    assert close(r["dpu"], pu.grad)
    assert R.blend_bwd(d["moe"], d["pu"], d["lat_w"], d["long_w"], d["out"], d["dout"], with_dpu=False)["dpu"] is None
    # float32, two orders
    r = R.blend_bwd(d["moe"], d["pu"], d["lat_w"], d["long_w"], d["out"], d["dout"])
    bb = R.blend_bwd_bounds(r, d["long_w"], d["lat_w"], B, kind)
    fb = R.blend_fwd_bounds(f)["out"]
    t = lambda v: v.to(F32)       # noqa: E731
    f32 = R.blend_fwd(t(d["moe"]), t(d["pu"]), t(d["lat_w"]), t(d["lat_b"]), t(d["long_w"]), t(d["long_b"]))["out"].to(F64)
    if kind == "lattice":
        assert eq(f32, f["out"].to(F32).to(F64)) and set(f32.flatten().tolist()) <= {0.0, 1.0, -1.0}
        assert (d["out"] == 0).any()
    else:
        assert ((f32 - f["out"]).abs() <= fb).all()
    for flip in (False, True):
        o = (lambda v: v.flip(0)) if flip else (lambda v: v)
        r32 = R.blend_bwd(o(t(d["moe"])), o(t(d["pu"])), t(d["lat_w"]), t(d["long_w"]), o(t(d["out"])), o(t(d["dout"])))
        assert ((r32["sums"].to(F64) - r["sums"]).abs() <= bb["sums"]).all()
        assert ((r32["dpu"].to(F64) - o(r["dpu"])).abs() <= o(bb["dpu"])).all()


def test_dice_reference_is_the_oracle():
    for case in R.DICE_CASES:
        B, C, HW, eps = case
        d = R.dice_data(case)
        r = R.dice_score(d["logits"], d["target"], eps)
        x4 = d["logits"].reshape(B, C, 1, HW)
        want = dice_oracle(x4.to(F32), d["target"].reshape(B, 1, HW), eps)
        got32 = R.dice_score(d["logits"].to(F32), d["target"], eps)
        assert torch.equal(got32["counts"], r["counts"]) and close(got32["dice"], want, 2.0 ** -22)
        assert close(r["dice"], want, 4 * 2.0 ** -24)
        hard = d["logits"].argmax(1)
        for c in range(C):
            assert r["counts"][:, c].tolist() == [int(((hard == c) & (d["target"] == c)).sum()), int((hard == c).sum()),
                                                  int((d["target"] == c).sum())]
        if C >= 3:
            assert r["counts"][1, C - 1] == 0 and r["counts"][2, C - 1] == 0          # a class absent from both
        if HW > 1:
            assert ((d["target"] < 0) | (d["target"] >= C)).any()
            assert r["counts"][2].sum() < B * HW
            srt = d["logits"].sort(1, descending=True).values
            assert C == 1 or (srt[:, 0] == srt[:, 1]).any()                           # ties


def test_dropout_table_is_the_hash_rule():
    seen = set()
    for N, C, p, seed in R.DROPOUT_CASES + [R.dropout_hit_case()]:
        t = R.dropout2d_table(N, C, p, seed)["table"]
        u = R.hash_uniform(seed, N * C).reshape(N, C)
        pf = float(torch.tensor(p, dtype=F32))
        scale = float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))) if p < 1 else 0.0
        assert eq(t, torch.where(u >= pf, torch.tensor(scale, dtype=F64), torch.zeros((), dtype=F64)))
        if p == 0:
            assert (t == 1).all()
        if p == 1:
            assert (t == 0).all()
        seen |= {N * C}
    assert seen >= {1, 256, 257, 1000}


@pytest.mark.parametrize("case", R.SCALE_CASES, ids=[R.case_id(c) for c in R.SCALE_CASES])
def test_channel_scale_reference(case):
    N, HW, C, win, dtype = case
    d = R.scale_data(case)
    r = R.channel_scale(d["x"], d["table"], C, d["coff"], dtype)
    co = d["coff"]
    v = d["x"][..., co:co + C]
    assert eq(r["x"][..., co:co + C], (v.to(F32) * d["table"][:, None].to(F32)).to(dtype).to(F64))       # float32 product, rounded once
    assert eq(torch.isnan(r["x"]), torch.isnan(d["x"])) and set(d["table"].flatten().tolist()) == set(R.TABLE_VALUES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the segmentation criterion

SEG_PARAMS = [pytest.param(s, k, id=f"{'x'.join(map(str, s))}-{k}") for s in R.SEG_SHAPES for k in R.KINDS]


def oracle_seg(x, t, mode):
    x = x.clone().requires_grad_(True)
    crit = O.AutoregressiveCriterion(n_target_frames=x.shape[1], loss_type=mode)
    loss = crit(x, t)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("shape,kind", SEG_PARAMS)
def test_seg_reference_is_the_oracle_criterion(shape, kind):
    B, F, C, H, W = shape
    for mode in R.SEG_MODES:
        d = R.seg_data(shape, kind, mode)
        x, t = d["logits"], d["target"]
        want, grad = oracle_seg(x, t, mode)
        r = R.seg_loss_fwd(x, t, mode, w_f32=True)
        assert close(r["loss"][0], want) and close(r["loss"][1:].sum(), r["loss"][0])
        for f in range(F):
            if mode == "tversky":
                assert close(r["loss"][1 + f], O.cross_entropy_tversky_weighted_loss(x[:, f], t[:, f]))
        b = R.seg_loss_bwd(x, t, r.get("coefG"), r.get("coefT"), None, mode)
        scale = grad.abs().max().clamp_min(1e-300)
        assert ((b["dlogits"] - grad).abs() <= 1e-12 * scale).all(), ((b["dlogits"] - grad).abs().max() / scale)
        b3 = R.seg_loss_bwd(x, t, r.get("coefG"), r.get("coefT"), -1.5, mode)
        assert close(b3["dlogits"], -1.5 * b["dlogits"])
        # float64 weights: the reference proper differs from the oracle's float32 weights by float32 rounding only
        r64 = R.seg_loss_fwd(x, t, mode)
        assert close(r64["loss"], r["loss"], 1e-5)


def test_seg_reference_with_other_weights_is_the_oracle_tversky():
    shape = R.SEG_SHAPES[4]
    d = R.seg_data(shape, "continuous")
    cw, tw, al, be = R.SEG_OTHER
    r = R.seg_loss_fwd(d["logits"], d["target"], "tversky", cw, tw, al, be)
    r0 = R.seg_loss_fwd(d["logits"], d["target"], "tversky")
    C, W = shape[2], shape[4]
    for f in range(shape[1]):
        tv = O.tversky_loss(d["logits"][:, f], d["target"][:, f], al, be)
        assert close(1 - r["ratio"][f].sum() / (C * W), tv)
        ce = (r0["loss"][1 + f] - 0.5 * O.tversky_loss(d["logits"][:, f], d["target"][:, f])) / 0.5
        assert close(r["loss"][1 + f], cw * ce + tw * tv, 1e-11)
    assert all(R.seg_conditions(r, shape, al, be).values())


@pytest.mark.parametrize("shape,kind", SEG_PARAMS)
def test_seg_inputs_and_float32_evaluation(shape, kind):
    B, F, C, H, W = shape
    d = R.seg_data(shape, kind)
    x, t = d["logits"], d["target"]
    r = R.seg_loss_fwd(x, t, "tversky")
    m = x.max(2, keepdim=True).values
    diff32 = (x.to(F32) - m.to(F32)).to(F64)
    assert eq(diff32, x - m)                                        # x - max is exact in float32
    assert not torch.isnan(r["loss"]).any() and (r["D"] > 0).all()
    if kind == "continuous":
        assert ((x - m) >= -16).all() and all(R.seg_conditions(r, shape).values()), R.seg_conditions(r, shape)
    else:
        top = x == m
        ntop = top.sum(2)
        assert ((ntop & (ntop - 1)) == 0).all() and ((x - m)[~top] == -256).all() and top.gather(2, t[:, :, None]).all()
        assert B * F * H * W < 8 or (r["partG"][:, 1] > 0).any()     # intersections: the class-dice weights see them
    bnd = R.seg_loss_bounds(r, shape, "tversky", kind)
    for flip in (False, True):
        o = (lambda v: v.flip(0).flip(-2)) if flip else (lambda v: v)
        r32 = R.seg_loss_fwd(o(x.to(F32)), o(t), "tversky")
        for name in ("partG", "partT", "coefG", "coefT", "loss"):
            err = (torch.nan_to_num(r32[name].to(F64), nan=NANV) - torch.nan_to_num(r[name], nan=NANV)).abs()
            assert (err <= bnd[name]).all(), (name, (err / bnd[name].clamp_min(1e-300)).max())
        if kind == "lattice":
            assert eq(r32["partT"].to(F64), r["partT"])
        for q in (0, 1, 3):
            assert eq(r32["partG"][:, q].to(F64), r["partG"][:, q])
    cG, cT = R.round_to(r["coefG"], F32), R.round_to(r["coefT"], F32)
    for dl in (None, -1.5):
        b = R.seg_loss_bwd(x, t, cG, cT, dl, "tversky")
        bb = R.seg_loss_bwd_bounds(b, shape, "tversky", kind, dl)["dlogits"]
        b32 = R.seg_loss_bwd(x.to(F32), t, cG.to(F32), cT.to(F32), dl, "tversky")["dlogits"].to(F64)
        assert ((b32 - b["dlogits"]).abs() <= bb).all()
    for mode in ("l1", "l2"):
        dm = R.seg_data(shape, kind, mode)
        rm = R.seg_loss_fwd(dm["logits"], dm["target"], mode)
        bm = R.seg_loss_bounds(rm, shape, mode, kind)
        for flip in (False, True):
            o = (lambda v: v.flip(0).flip(-1)) if flip else (lambda v: v)
            r32 = R.seg_loss_fwd(o(dm["logits"].to(F32)), o(dm["target"]), mode)
            assert ((r32["partG"].to(F64) - rm["partG"]).abs() <= bm["partG"]).all()
            assert ((r32["loss"].to(F64) - rm["loss"]).abs() <= bm["loss"]).all()
            if kind == "lattice":
                assert eq(r32["partG"].to(F64), rm["partG"])
        if kind == "lattice" and mode == "l1" and B * F * C * H * W > 64:
            oh = Fn.one_hot(dm["target"], C).movedim(-1, 2)
            assert (dm["logits"] == oh).any()                         # the L1 gradient is 0 there


def test_seg_geometry_and_routes():
    lib = hip.load()
    for B, H, W in [(1, 1, 1), (2, 3, 5), (2, 5, 256), (1, 7, 257), (2, 33, 9), (1, 3, 300), (1, 2049, 2048), (3, 64, 513)]:
        assert lib.pmoe_seg_loss_rows(B, H, W) == R.seg_loss_rows(B, H, W) == min(B * H, 64) * -(-W // 256)
    for C in range(0, 35):
        assert lib.pmoe_seg_loss_cp(C) == R.seg_loss_cp(C)
    cps = [R.seg_loss_cp(s[2]) for s in R.SEG_SHAPES]
    assert cps == [8, 8, 16, 16, 24, 24, 32, 32]
    assert {s[2] for s in R.SEG_SHAPES} >= {8, 16, 24, 32}                       # C == CP: no padded lane
    assert sum(R.seg_geometry(s[0], s[3], s[4], s[2])["xb"] > 1 for s in R.SEG_SHAPES) >= 2       # more than one column block
    assert any(s[0] * s[3] > 64 for s in R.SEG_SHAPES) and any(s[4] % 256 == 0 for s in R.SEG_SHAPES)
    B, F, C, H, W = R.SEG_BIG
    assert R.grid_stride_entered(B * F * H * W, R.GRID_CAPS["seg_loss_bwd"])
    g = R.seg_geometry(B, H, W, C)
    assert (g["xb"], g["nsplit"]) == (8, 64)


def test_every_case_that_claims_a_route_takes_it():
    routes = [R.window_route(*c[1:]) for c in R.WINDOW_CASES]
    assert routes == ["vector", "scalar", "scalar", "scalar", "scalar"] * 4
    for c in R.WINDOW_CASES:                      # each scalar case for one reason alone
        rows, C, sld, sco, dld, dco, dtype = c
        v = R.ve(dtype)
        assert sum([C % v != 0, sco % v != 0, dco % v != 0, sld % v != 0 or dld % v != 0]) == (0 if R.window_route(*c[1:]) == "vector" else 1)
    cat = [R.cat_route(c[2], c[4], c[7]) for c in R.CAT_CASES]
    assert cat == (["lds"] * 14 + ["element"] * 2) * 2
    K, cc, sld, sco, dst_c, dst_ld, rows, dtype = R.CAT_CASES[15]
    assert sld % R.ve(dtype) == 0 and 32 * dst_c * R.esize(dtype) > 48 * 1024 >= 32 * (dst_c - R.ve(dtype)) * R.esize(dtype)
    assert {c[6] for c in R.CAT_CASES} >= {1, 31, 32, 33} and any(c[3] % R.ve(c[7]) for c in R.CAT_CASES)
    # the i += 256 loops and the second workgroup
    assert any(2 * B > 256 for B in R.B_CASES) and any(B > 256 for B in R.B_CASES) and any(R.chain256(B) == 3 for B in R.B_CASES)
    for name, (items, _) in R.BIG_CASES.items():
        assert R.grid_stride_entered(items, R.GRID_CAPS[name.split("/")[0]]) and items % 256, name
    B, C, HW, _ = R.DICE_BIG
    assert R.grid_stride_entered(B * HW, R.GRID_CAPS["dice_count"])
    assert 64 * (R.NCHW_MAX_C + 1) * 4 == 160 * 1024 and any(c[2] == R.NCHW_MAX_C for c in R.NCHW_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants

def caught_exact(ref, mutant):
    return not eq(ref, mutant)


def caught_bound(ref, mutant, bound):
    return bool(((torch.nan_to_num(ref, nan=NANV) - torch.nan_to_num(mutant, nan=NANV)).abs() >= 16 * bound.clamp_min(1e-300)).any()) and \
        not eq(ref, mutant)


def _pool(mut, out):
    for case in R.POOL_CASES:
        d = R.pool_data(case)
        H, W = d["x"].shape[1:3]
        if out == "y":
            yield caught_exact(R.maxpool2s2_fwd(d["x"], d["C"], d["x_coff"])["y"], R.maxpool2s2_fwd(d["x"], d["C"], d["x_coff"], mut)["y"])
        elif not (H % 2 or W % 2):
            a = (d["x"], d["dy"], d["dskip"], d["C"], d["x_coff"], d["ds_coff"], case[-1])
            yield caught_exact(R.maxpool2s2_bwd(*a)["dx"], R.maxpool2s2_bwd(*a, mut)["dx"])


def _shuffle(mut):
    for case in R.SHUFFLE_CASES:
        src, C, dld, dco = shuffle_src(case)
        dst = R.pixel_shuffle2(src, C, dld, dco)["dst"]
        yield caught_exact(dst, R.pixel_shuffle2(src, C, dld, dco, mut)["dst"]) and \
            caught_exact(R.pixel_unshuffle2(dst, C, dco, src.shape[-1])["dst"], R.pixel_unshuffle2(dst, C, dco, src.shape[-1], mut)["dst"])


def _windows(mut):
    for case in R.WINDOW_CASES:
        rows, C, sld, sco, dld, dco, dtype = case
        d = R.window_data(case)
        if sco:
            yield caught_exact(R.copy_window(d["src"], sco, dld, dco, C)["dst"], R.copy_window(d["src"], sco, dld, dco, C, mut)["dst"]) and \
                caught_exact(R.add_window(d["src"], sco, d["dst"], dco, C, dtype)["dst"], R.add_window(d["src"], sco, d["dst"], dco, C, dtype, mut)["dst"])
    for case in R.NCHW_CASES:
        N, HW, C, ld, coff, dtype = case
        if coff:
            src = R.nchw_data(case)["src"]
            yield caught_exact(R.nhwc_to_nchw(src, C, coff)["dst"], R.nhwc_to_nchw(src, C, coff, mut)["dst"])
    for case in R.SCALE_CASES:
        d = R.scale_data(case)
        if d["coff"]:
            yield caught_exact(R.channel_scale(d["x"], d["table"], case[2], d["coff"], case[4])["x"],
                               R.channel_scale(d["x"], d["table"], case[2], d["coff"], case[4], mut)["x"])
    yield any(_pool(mut, "y")) and any(_pool(mut, "dx"))


def _cat(mut):
    for case in R.CAT_CASES:
        K, c, sld, sco, dst_c, dst_ld, rows, dtype = case
        srcs = R.cat_data(case)["srcs"]
        yield caught_exact(R.cat_windows(srcs, c, sco, dst_ld, dst_c)["dst"], R.cat_windows(srcs, c, sco, dst_ld, dst_c, mut)["dst"])


def _seg(mut, names, modes=("tversky",), bwd=False):
    for shape in R.SEG_SHAPES:
        for kind in R.KINDS:
            for mode in modes:
                d = R.seg_data(shape, kind, mode)
                r = R.seg_loss_fwd(d["logits"], d["target"], mode)
                if bwd:
                    cG, cT = r.get("coefG"), r.get("coefT")
                    b, m = (R.seg_loss_bwd(d["logits"], d["target"], cG, cT, None, mode, mu)["dlogits"] for mu in ("", mut))
                    yield caught_exact(b, m) if kind == "lattice" else False
                    continue
                m = R.seg_loss_fwd(d["logits"], d["target"], mode, mut=mut)
                bnd = R.seg_loss_bounds(r, shape, mode, kind)
                yield any(caught_bound(r[n], m[n], bnd[n]) for n in names)


def _loss(mut):
    for case in R.LOSS_CASES:
        for kind in R.KINDS:
            d = R.loss_data(case, kind)
            a = (d["actions"], d["speeds"], d["gt"], d["spd_gt"], *R.LOSS_C, case[0])
            r, m = R.action_loss(*a), R.action_loss(*a, mut)
            b = R.action_loss_bounds(r, *R.LOSS_C, case[0], kind)
            yield caught_bound(r["dact"], m["dact"], b["dact"]) and (mut == "l1sign" or caught_bound(r["loss"], m["loss"], b["loss"]))


def _blend(mut):
    for B in R.BLEND_CASES:
        for kind in R.KINDS:
            d = R.blend_data(B, kind)
            a = (d["moe"], d["pu"], d["lat_w"], d["long_w"], d["out"], d["dout"])
            r, m = R.blend_bwd(*a), R.blend_bwd(*a, mut=mut)
            b = R.blend_bwd_bounds(r, d["long_w"], d["lat_w"], B, kind)
            yield caught_exact(r["dpu"], m["dpu"]) if kind == "lattice" else caught_bound(r["dpu"], m["dpu"], b["dpu"])


def _dice(mut):
    for case in R.DICE_CASES:
        d = R.dice_data(case)
        r, m = R.dice_score(d["logits"], d["target"], case[3]), R.dice_score(d["logits"], d["target"], case[3], mut)
        yield not torch.equal(r["counts"], m["counts"]) or caught_bound(r["dice"], m["dice"], 4 * R.EPS24 * r["dice"].abs())


def _dropout(mut):
    for N, C, p, seed in R.DROPOUT_CASES + [R.dropout_hit_case()]:
        yield caught_exact(R.dropout2d_table(N, C, p, seed)["table"], R.dropout2d_table(N, C, p, seed, mut)["table"])


MUTANTS = {
    "pool: last maximum wins": lambda: _pool("last", "dx"),
    "pool: NaN dropped": lambda: _pool("nan", "y"),
    "pool backward: skip gradient dropped": lambda: _pool("skip", "dx"),
    "shuffle: quadrant transposed": lambda: _shuffle("quad"),
    "a window offset ignored": lambda: _windows("coff"),
    "cat: pad not zeroed": lambda: _cat("pad"),
    "cat: a source vector's overhang leaks": lambda: _cat("leak"),
    "cat: source offset ignored": lambda: _cat("coff"),
    "seg: soft-max over the padded lanes": lambda: _seg("padded", ("partT", "loss")),
    "seg: Tversky reduced over columns": lambda: _seg("cols", ("coefT", "loss")),
    "seg: class-dice weight without intersection": lambda: _seg("nointer", ("coefG", "loss")),
    "seg: CE normalised by the pixel count": lambda: _seg("cenorm", ("coefG", "loss")),
    "seg: coefT terms swapped": lambda: _seg("coefswap", ("coefT",)),
    "seg: L1 sign at zero": lambda: _seg("l1sign", (), ("l1",), bwd=True),
    "action_loss: L1 sign at zero": lambda: _loss("l1sign"),
    "action_loss: 1/B for 1/(2B)": lambda: _loss("halfB"),
    "blend: dpunet with w[0]": lambda: _blend("w0"),
    "dice: union without eps": lambda: _dice("noeps"),
    "dice: highest index on ties": lambda: _dice("last"),
    "dropout: counter c for n*C + c": lambda: _dropout("ctr"),
    "dropout: > for >=": lambda: _dropout("gt"),
    "dropout: keep_scale missing": lambda: _dropout("noscale"),
}


@pytest.mark.parametrize("name", list(MUTANTS), ids=lambda n: n.replace(" ", "_"))
def test_every_mutant_is_caught(name):
    hits = list(MUTANTS[name]())
    assert any(hits), f"{name}: no case catches it"


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals this revision adds: pmoe_nhwc_to_nchw refuses the channel counts whose [64][C + 1] float32 tile exceeds the 160 KiB that
# the launch opts in to (made-up pointers: a refused call dereferences nothing)

def test_nhwc_to_nchw_refuses_what_the_launch_cannot_hold():
    lib = hip.load()
    for C in (R.NCHW_MAX_C + 1, 1024, 1025):
        assert ER.call(lib, "pmoe_nhwc_to_nchw", [ER.p1, 4096, 0, ER.p2, 2, 64, C, 0, None]) == -1
    assert R.NCHW_MAX_C == 639
