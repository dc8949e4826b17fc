"""The U-Net, segmentation-loss and action-head kernels of csrc/punet.hip, csrc/stage1.hip and csrc/stage0.hip, each against the
float64 reference of its own operation (tests/unet_ref.py), through pmoe_amd.ops.  Every kernel gets the REFERENCE's inputs, never
another kernel's output; outputs are NaN-filled (sentinel-filled where NaN is data) before the launch and compared whole, what lies
outside a channel window and beyond the batch included; inputs must come back unmodified.

  exact       pool, shuffle, channel windows, concatenation, layout, Dropout2d, every count: bit for bit in both storage types
  lattice     inputs on which float32 arithmetic is exact in any order (tests/test_unet_kernels_cpu.py proves it of every generator)
  continuous  bounds from float32 rounding and the measured error of the device's tanhf / expf / logf, written out in unet_ref;
              every comparison prints max err / bound
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import ops  # noqa: E402
from tests import unet_ref as R  # noqa: E402
from tests.test_eca_head_gpu import dev, filled, refused, same_bits, same_with_nan, unchanged, within  # noqa: E402

DEV = "cuda"
F64, F32, BF16 = R.F64, R.F32, R.BF16
SENTINEL = -77.0
I64 = torch.int64


def ids(cases):
    return [R.case_id(c) for c in cases]


def whole(got, ref, dtype, what):
    """the whole buffer bit for bit; NaN where and only where the reference holds it (a NaN's payload apart)"""
    same_with_nan(got, ref, what)
    g = got.detach().cpu()
    same_bits(torch.where(torch.isnan(g), torch.zeros((), dtype=g.dtype), g), torch.nan_to_num(ref, nan=0.0), dtype, what)


def bounded(got, ref, bound, what):
    """|got - ref| <= bound element by element, NaN where and only where the reference holds it; prints max err / bound"""
    g = got.detach().cpu().to(F64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(ref.shape)}"
    assert torch.equal(torch.isnan(g), torch.isnan(ref)), f"{what}: unwritten elements, or written where nothing belongs"
    within(torch.nan_to_num(g), torch.nan_to_num(ref), torch.as_tensor(bound, dtype=F64).expand_as(ref), "continuous", what)


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# MaxPool2d(2, 2)

@pytest.mark.parametrize("case", R.POOL_CASES, ids=ids(R.POOL_CASES))
def test_maxpool2_fwd_bwd(case):
    N, H, W, cv, xwin, skip, dtype = case
    d = R.pool_data(case)
    C, co = d["C"], d["x_coff"]
    xd = dev(d["x"], dtype)
    y = filled((N, H // 2, W // 2, C), dtype, SENTINEL)
    ops.maxpool2_fwd(xd, y, C, co)
    sync()
    whole(y, R.maxpool2s2_fwd(d["x"], C, co)["y"], dtype, "maxpool2 y")
    if not (H % 2 or W % 2):
        dyd, dsd = dev(d["dy"], dtype), dev(d["dskip"], dtype)
        dx = filled((N, H, W, C), dtype)
        ops.maxpool2_bwd(xd, dyd, dx, dsd, C, co, d["ds_coff"])
        sync()
        whole(dx, R.maxpool2s2_bwd(d["x"], d["dy"], d["dskip"], C, co, d["ds_coff"], dtype)["dx"], dtype, "maxpool2 dx")
        unchanged({"dy": (dyd, d["dy"]), "dskip": (dsd, d["dskip"])})
    unchanged({"x": (xd, d["x"])})


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_maxpool2_forward_gives_nan_where_its_backward_routes_the_gradient_to_one(dtype):
    C = R.ve(dtype)
    x = torch.tensor([[1.0, R.NAN], [2.0, 0.5]], dtype=F64)[None, :, :, None].repeat(1, 1, 1, C)        # one NaN, tap 1
    x[..., 1] = torch.tensor([[R.NAN, 3.0], [R.NAN, 0.5]], dtype=F64)                                 # two NaNs: the last one
    xd, y, dx = dev(x, dtype), filled((1, 1, 1, C), dtype, SENTINEL), filled((1, 2, 2, C), dtype)
    ops.maxpool2_fwd(xd, y)
    ops.maxpool2_bwd(xd, dev(torch.ones(1, 1, 1, C, dtype=F64), dtype), dx)
    sync()
    assert torch.isnan(y).all(), "a NaN in the window must give NaN, as in torch.max_pool2d"
    want = torch.zeros(1, 2, 2, C, dtype=F64)
    want[0, 0, 1, :], want[0, 0, 1, 1], want[0, 1, 0, 1] = 1.0, 0.0, 1.0
    whole(dx, want, dtype, "gradient at the NaN")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_fused_bn_pool_keeps_a_nan_like_the_stand_alone_pool(dtype):
    """pmoe_bn_apply_pool2 is documented as bit-identical to pmoe_bn_apply + pmoe_maxpool2s2_fwd: with scale 1, shift 0, mean 0 and
    no ReLU its y is x, and its pooled tensor must be the stand-alone pool of the planted windows, NaN included"""
    case = (2, 6, 10, 1, False, "null", dtype)
    d = R.pool_data(case)
    N, H, W, C = d["x"].shape
    x = d["x"]
    xd = dev(x, dtype)
    y, pooled = filled((N, H, W, C), dtype, SENTINEL), filled((N, H // 2, W // 2, C), dtype, SENTINEL)
    one, zero = torch.ones(1, C, device=DEV), torch.zeros(1, C, device=DEV)
    ops.bn_apply_pool2(xd, y, pooled, one, zero, zero, N, 1, C, False)
    sync()
    whole(y, x, dtype, "bn_apply_pool2 y")
    ref = R.maxpool2s2_fwd(x, C)["y"]
    assert torch.isnan(ref).any()
    whole(pooled, ref, dtype, "bn_apply_pool2 pooled")


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel shuffle / unshuffle

def shuffle_src(case):
    N, H, W, cv, extra, dmul, doff, dtype = case
    C = cv * R.ve(dtype)
    src = R.nanlike((N, H, W, 4 * C + extra * R.ve(dtype)))
    src[..., :4 * C] = R.lat(R.gen("shuffle", case), (N, H, W, 4 * C), 64, 4)
    return src, C, dmul * C, doff * C


@pytest.mark.parametrize("case", R.SHUFFLE_CASES, ids=ids(R.SHUFFLE_CASES))
def test_pixel_shuffle2_unshuffle2(case):
    dtype = case[-1]
    src, C, dld, dco = shuffle_src(case)
    N, H, W, sld = src.shape
    ref = R.pixel_shuffle2(src, C, dld, dco)["dst"]
    sd, dst = dev(src, dtype), filled((N, 2 * H, 2 * W, dld), dtype)
    ops.pixel_shuffle2(sd, dst, C, dco)
    sync()
    whole(dst, ref, dtype, "pixel_shuffle2")
    rd, back = dev(ref, dtype), filled((N, H, W, sld), dtype)
    ops.pixel_unshuffle2(rd, back, C, dco)
    sync()
    whole(back, R.pixel_unshuffle2(ref, C, dco, sld)["dst"], dtype, "pixel_unshuffle2")
    whole(back, src, dtype, "unshuffle(shuffle(src))")
    unchanged({"src": (sd, src), "shuffled": (rd, ref)})


# ---------------------------------------------------------------------------------------------------------------------------------
# channel windows

@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=ids(R.WINDOW_CASES))
def test_copy_window_add_window(case):
    rows, C, sld, sco, dld, dco, dtype = case
    d = R.window_data(case)
    sd, dst = dev(d["src"], dtype), filled((rows, dld), dtype)
    ops.copy_window(sd, sco, dst, dco, C)
    sync()
    whole(dst, R.copy_window(d["src"], sco, dld, dco, C)["dst"], dtype, f"copy_window {R.window_route(*case[1:])}")
    acc = dev(d["dst"], dtype)
    ops.add_window(sd, sco, acc, dco, C)
    sync()
    whole(acc, R.add_window(d["src"], sco, d["dst"], dco, C, dtype)["dst"], dtype, f"add_window {R.window_route(*case[1:])}")
    unchanged({"src": (sd, d["src"])})


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_window_of_no_rows_returns_0_and_writes_nothing(dtype):
    v = R.ve(dtype)
    src, dst = filled((2, v), dtype, 1.0), filled((2, v), dtype)
    lib = ops.load()
    for fn in (lib.pmoe_copy_window, lib.pmoe_add_window):
        assert fn(ops.ptr(src, "src"), v, 0, ops.ptr(dst, "dst"), v, 0, 0, v, ops.dt(src), ops.stream_ptr()) == 0
    sync()
    assert torch.isnan(dst).all()


@pytest.mark.parametrize("case", R.CAT_CASES, ids=ids(R.CAT_CASES))
def test_cat_windows(case):
    K, c, sld, sco, dst_c, dst_ld, rows, dtype = case
    srcs = R.cat_data(case)["srcs"]
    sd = [dev(s, dtype) for s in srcs]
    dst = filled((rows, dst_ld), dtype)
    ops.cat_windows(sd, dst, c, sco, dst_c)
    sync()
    whole(dst, R.cat_windows(srcs, c, sco, dst_ld, dst_c)["dst"], dtype, f"cat_windows {R.cat_route(sld, dst_c, dtype)}")
    unchanged({f"src{k}": (sd[k], srcs[k]) for k in range(K)})


@pytest.mark.parametrize("case", R.NCHW_CASES, ids=ids(R.NCHW_CASES))
def test_nhwc_to_nchw(case):
    N, HW, C, ld, coff, dtype = case
    src = R.nchw_data(case)["src"]
    sd, dst = dev(src, dtype), filled((N, C, 1, HW))
    ops.nhwc_to_nchw(sd, dst, C, coff)
    sync()
    whole(dst, R.nhwc_to_nchw(src, C, coff)["dst"], F32, "nhwc_to_nchw")
    unchanged({"src": (sd, src)})


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.tname)
def test_nhwc_to_nchw_serves_its_largest_channel_count_and_refuses_the_next(dtype):
    C = R.NCHW_MAX_C
    src = R.lat(R.gen("nchw max", dtype), (1, 1, 70, C), 64, 4)
    sd, dst = dev(src, dtype), filled((1, C, 1, 70))
    ops.nhwc_to_nchw(sd, dst, C)
    sync()
    whole(dst, R.nhwc_to_nchw(src, C, 0)["dst"], F32, "nhwc_to_nchw, largest C")
    refused(ops.nhwc_to_nchw, filled((1, 1, 1, C + 1), dtype, 0.0), filled((1, C + 1, 1, 1)), C + 1)
    refused(ops.nhwc_to_nchw, filled((1, 1, 1, 1024), dtype, 0.0), filled((1, 1024, 1, 1)), 1024)


# ---------------------------------------------------------------------------------------------------------------------------------
# grid-stride loops: more items than cap x 256 and a ragged tail; float32 lattice values, every result exact

def big_lat(shape, lim=8):
    g = torch.Generator(device=DEV).manual_seed(len(shape) * 1000 + lim)
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g, device=DEV).to(F32) / 4


def big_taps(x):
    return [x[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]


def test_grid_stride_maxpool2():
    p = R.BIG_CASES["maxpool2_fwd"][1]
    x = big_lat((p["N"], p["H"], p["W"], p["C"]))
    y = filled((p["N"], p["H"] // 2, p["W"] // 2, p["C"]))
    ops.maxpool2_fwd(x, y)
    t = big_taps(x)
    m, best = t[0], torch.zeros(t[0].shape, dtype=torch.int8, device=DEV)
    for q in (1, 2, 3):
        take = t[q] > m
        m, best = torch.where(take, t[q], m), torch.where(take, torch.full_like(best, q), best)
    assert torch.equal(y, m), "maxpool2 forward, grid-stride"
    shape = m.shape
    del y, m, t, take
    dy = big_lat(shape, 7) + 0.125
    dx = filled(x.shape)
    ops.maxpool2_bwd(x, dy, dx)
    for q in range(4):
        assert torch.equal(dx[:, q >> 1::2, q & 1::2], torch.where(best == q, dy, torch.zeros((), device=DEV))), \
            "maxpool2 backward, grid-stride"


def test_grid_stride_pixel_shuffle2_unshuffle2():
    p = R.BIG_CASES["pixel_shuffle2"][1]
    N, H, W, C = p["N"], p["H"], p["W"], p["C"]
    src = big_lat((N, H, W, 4 * C), 64)
    dst = filled((N, 2 * H, 2 * W, C))
    ops.pixel_shuffle2(src, dst, C)
    for q in range(4):
        assert torch.equal(dst[:, q >> 1::2, q & 1::2], src[..., q * C:(q + 1) * C]), "pixel_shuffle2, grid-stride"
    back = filled(src.shape)
    ops.pixel_unshuffle2(dst, back, C)
    assert torch.equal(back, src), "pixel_unshuffle2, grid-stride"


@pytest.mark.parametrize("form", ("vector", "scalar"))
def test_grid_stride_copy_window_add_window(form):
    p = R.BIG_CASES[f"copy_window/{form}"][1]
    assert R.window_route(p["C"], p["ld"], 0, p["ld"], 0, F32) == form
    src = big_lat((p["rows"], p["ld"]), 64)
    dst = filled(src.shape)
    ops.copy_window(src, 0, dst, 0, p["C"])
    assert torch.equal(dst, src), "copy_window, grid-stride"
    acc = big_lat(src.shape, 63)
    before = acc.clone()
    ops.add_window(src, 0, acc, 0, p["C"])
    assert torch.equal(acc, before + src), "add_window, grid-stride"


def test_grid_stride_cat_windows_element_wise():
    p = R.BIG_CASES["cat_windows"][1]
    assert R.cat_route(p["src_ld"], p["dst_c"], F32) == "element"
    src = big_lat((p["rows"], p["src_ld"]), 64)
    dst = filled((p["rows"], p["dst_c"]))
    ops.cat_windows([src], dst, p["c"], 1, p["dst_c"])
    assert torch.equal(dst[:, :3], src[:, 1:4]) and (dst[:, 3] == 0).all(), "cat_windows, grid-stride"


def test_grid_stride_channel_scale():
    p = R.BIG_CASES["channel_scale"][1]
    x = big_lat((p["N"], 1, p["HW"], p["C"]), 64)
    table = torch.tensor([[0.0, 2.0, 0.5, -1.25]], device=DEV)
    before = x.clone()
    ops.channel_scale(x, table)
    assert torch.equal(x, before * table[:, None, None, :]), "channel_scale, grid-stride"


# ---------------------------------------------------------------------------------------------------------------------------------
# Dropout2d, dice

@pytest.mark.parametrize("case", R.DROPOUT_CASES + [R.dropout_hit_case()], ids=lambda c: "-".join(map(str, c)))
def test_dropout2d_table_is_the_hash(case):
    N, C, p, seed = case
    table = filled((N + 1, C))
    ops.dropout2d_table(table[:N], p, seed)
    sync()
    ref = torch.cat([R.dropout2d_table(N, C, p, seed)["table"], R.nanlike((1, C))])
    whole(table, ref, F32, "dropout2d_table")


@pytest.mark.parametrize("case", R.SCALE_CASES, ids=ids(R.SCALE_CASES))
def test_channel_scale(case):
    N, HW, C, win, dtype = case
    d = R.scale_data(case)
    x = dev(d["x"][:, None], dtype)
    td = dev(d["table"])
    ops.channel_scale(x, td, C, d["coff"])
    sync()
    whole(x[:, 0], R.channel_scale(d["x"], d["table"], C, d["coff"], dtype)["x"], dtype, "channel_scale")
    unchanged({"table": (td, d["table"])})


def check_dice(case, what):
    B, C, HW, eps = case
    d = R.dice_data(case)
    ref = R.dice_score(d["logits"], d["target"], eps)
    xd, td = dev(d["logits"].reshape(B, C, 1, HW)), d["target"].reshape(B, 1, HW).to(DEV)
    dice, counts = ops.dice_score(xd, td, eps)
    sync()
    assert torch.equal(counts.cpu(), ref["counts"]), f"{what}: counts differ"
    bounded(dice, ref["dice"], 4 * R.EPS24 * ref["dice"].abs(), what)
    unchanged({"logits": (xd, d["logits"].reshape(B, C, 1, HW))})
    assert torch.equal(td.cpu().reshape(B, HW), d["target"])
    return dice, counts


@pytest.mark.parametrize("case", R.DICE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dice_score_counts_and_quotient(case):
    check_dice(case, "dice")


def test_dice_score_beyond_one_pass_of_the_grid_is_reproducible():
    a, b = check_dice(R.DICE_BIG, "dice, grid-stride"), check_dice(R.DICE_BIG, "dice, grid-stride again")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# action head, action loss, blend

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=ids(R.HEAD_CASES))
def test_action_head_fwd_bwd(case, kind):
    B, hld, sld, dtype = case
    d = R.head_data(case, kind)
    rows = d["rows"]
    hd, sd = dev(d["head"], dtype), dev(d["spd"], dtype)
    actions, speeds = filled((rows, 2)), filled((rows,))
    ops.action_head_fwd(hd, sd, actions, speeds, B)
    sync()
    ref = R.action_head_fwd(d["head"], d["spd"], B)
    pad = R.nanlike((rows - B, 2))
    if kind == "lattice":
        whole(actions, torch.cat([ref["actions"].to(F32).to(F64), pad]), F32, "actions")
    else:
        bounded(actions, torch.cat([ref["actions"], pad]), torch.cat([R.action_head_fwd_bounds(ref)["actions"], pad.nan_to_num()]),
                "action_head_fwd actions")
    whole(speeds, torch.cat([ref["speeds"], pad[:, 0]]), F32, "speeds")
    unchanged({"head": (hd, d["head"]), "spd": (sd, d["spd"])})
    ad = dev(d["actions"])
    for null in ("none", "dactions", "dspeeds"):
        da = None if null == "dactions" else d["dact"]
        ds = None if null == "dspeeds" else d["dspeeds"]
        dad, dsd = dev(da), dev(ds)
        dhead, dspd = filled((rows, hld), dtype), filled((rows, sld), dtype)
        ops.action_head_bwd(ad, dad, dsd, dhead, dspd, B)
        sync()
        r = R.action_head_bwd(d["actions"], da, ds, rows, hld, sld, B, dtype)
        if kind == "lattice" or dtype == BF16:
            whole(dhead, r["dhead"], dtype, f"dhead, null {null}")
        else:
            b = torch.zeros(rows, hld, dtype=F64)
            b[:B, :2] = R.stored_bound(r["raw"], r["mag"])
            bounded(dhead, r["dhead"], b, f"action_head_bwd dhead, null {null}")
        whole(dspd, r["dspd"], dtype, f"dspd, null {null}")
        unchanged({"actions": (ad, d["actions"]), "dactions": (dad, da), "dspeeds": (dsd, ds)})


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=ids(R.LOSS_CASES))
def test_action_loss(case, kind):
    B, ws = case
    d = R.loss_data(case, kind)
    c0, c1 = R.LOSS_C
    ref = R.action_loss(d["actions"], d["speeds"], d["gt"], d["spd_gt"], c0, c1, B)
    bnd = R.action_loss_bounds(ref, c0, c1, B, kind)
    ins = {k: dev(d[k]) for k in ("actions", "speeds", "gt", "spd_gt")}
    loss, dact, dsp = filled((2,)), filled((B + 1, 2)), filled((B + 1,))
    ops.action_loss(ins["actions"], ins["speeds"], ins["gt"], ins["spd_gt"], c0, c1, loss, dact, dsp if ws else None, B)
    sync()
    bounded(loss, torch.stack([ref["loss"], torch.tensor(R.NAN, dtype=F64)]), torch.stack([bnd["loss"], torch.zeros((), dtype=F64)]),
            f"action_loss loss {kind}")
    pad = R.nanlike((1, 2))
    bounded(dact, torch.cat([ref["dact"], pad]), torch.cat([bnd["dact"], pad.nan_to_num()]), f"action_loss dactions {kind}")
    assert (dact[:B].cpu()[d["actions"] == d["gt"]] == 0).all()
    if ws:
        bounded(dsp, torch.cat([ref["dspeeds"], pad[0, :1]]), torch.cat([bnd["dspeeds"], torch.zeros(1, dtype=F64)]),
                f"action_loss dspeeds {kind}")
    else:
        assert torch.isnan(dsp).all()
    unchanged({k: (ins[k], d[k]) for k in ins})


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B", R.BLEND_CASES)
def test_blend_fwd_bwd(B, kind):
    d = R.blend_data(B, kind)
    names = ("moe", "pu", "lat_w", "lat_b", "long_w", "long_b", "out", "dout")
    dd = {k: dev(d[k]) for k in names}
    out = filled((B + 1, 2))
    ops.blend_fwd(dd["moe"], dd["pu"], dd["lat_w"], dd["lat_b"], dd["long_w"], dd["long_b"], out, B)
    sync()
    ref = R.blend_fwd(d["moe"], d["pu"], d["lat_w"], d["lat_b"], d["long_w"], d["long_b"])
    pad = R.nanlike((1, 2))
    if kind == "lattice":
        whole(out, torch.cat([ref["out"].to(F32).to(F64), pad]), F32, "blend out")
    else:
        bounded(out, torch.cat([ref["out"], pad]), torch.cat([R.blend_fwd_bounds(ref)["out"], pad.nan_to_num()]), "blend_fwd out")
    for with_dpu in (True, False):
        g = {k: filled((n,)) for k, n in (("dlat_w", 2), ("dlat_b", 1), ("dlong_w", 2), ("dlong_b", 1))}
        dpu = filled((B + 1, 2))
        ops.blend_bwd(dd["moe"], dd["pu"], dd["lat_w"], dd["long_w"], dd["out"], dd["dout"], g["dlat_w"], g["dlat_b"], g["dlong_w"],
                      g["dlong_b"], dpu if with_dpu else None, B)
        sync()
        r = R.blend_bwd(d["moe"], d["pu"], d["lat_w"], d["long_w"], d["out"], d["dout"], with_dpu)
        bnd = R.blend_bwd_bounds(r, d["long_w"], d["lat_w"], B, kind)
        got = torch.stack([torch.cat([g["dlat_w"], g["dlat_b"]]), torch.cat([g["dlong_w"], g["dlong_b"]])])
        bounded(got, r["sums"], bnd["sums"], f"blend_bwd sums {kind}")
        if with_dpu:
            bounded(dpu, torch.cat([r["dpu"], pad]), torch.cat([bnd["dpu"], pad.nan_to_num()]), f"blend_bwd dpunet {kind}")
        else:
            assert torch.isnan(dpu).all()
    unchanged({k: (dd[k], d[k]) for k in names})


# ---------------------------------------------------------------------------------------------------------------------------------
# segmentation criterion

def seg_launch(x, t, mode, weights=R.SEG_DEFAULTS):
    """pmoe_seg_loss_fwd with NaN-filled buffers of exactly the sizes the kernels index -> (loss, coefG, coefT, partG, partT)"""
    B, F, C, H, W = x.shape
    geo, CP = R.seg_geometry(B, H, W, C), R.seg_loss_cp(C)
    lib = ops.load()
    assert lib.pmoe_seg_loss_rows(B, H, W) == geo["NS"] and lib.pmoe_seg_loss_cp(C) == CP
    partG, loss = filled((F, geo["NS"], 4, 32)), filled((1 + F,))
    tv = mode == "tversky"
    partT = filled((F, geo["nsplit"], 3, CP, W)) if tv else None
    coefG, coefT = (filled((F, 32)), filled((F, 2, CP, W))) if tv else (None, None)
    p = lambda v: None if v is None else ops.ptr(v, "buffer", F32)       # noqa: E731
    ops.check(lib.pmoe_seg_loss_fwd(ops.ptr(x, "logits", F32), ops.ptr(t, "target", I64), B, F, C, H, W, ops.SEG_MODES[mode], *weights,
                                    p(partT), p(partG), p(coefG), p(coefT), p(loss), ops.stream_ptr()), "pmoe_seg_loss_fwd")
    sync()
    return loss, coefG, coefT, partG, partT


def check_seg_fwd(shape, kind, mode, x, t, what):
    ref = R.seg_loss_fwd(x, t, mode)
    bnd = R.seg_loss_bounds(ref, shape, mode, kind)
    xd, td = dev(x), t.to(DEV)
    loss, coefG, coefT, partG, partT = seg_launch(xd, td, mode)
    G = partG.cpu().to(F64).sum(1)
    assert not torch.isnan(G).any(), "partG: unwritten rows"
    if mode == "tversky":
        for q in (0, 1, 3):
            assert torch.equal(G[:, q], ref["partG"][:, q]), f"{what}: counts q = {q} differ"
        bounded(G[:, 2], ref["partG"][:, 2], bnd["partG"][:, 2], f"{what} partG -log p_t")
        T = partT.cpu().to(F64).sum(1)
        assert torch.equal(T[:, 0], ref["partT"][:, 0]), f"{what}: target counts per column differ"
        if kind == "lattice":
            assert torch.equal(T[:, 1:], R.round_to(ref["partT"][:, 1:], F32)), f"{what}: partT not exact on the lattice"
        else:
            bounded(T[:, 1:], ref["partT"][:, 1:], bnd["partT"][:, 1:], f"{what} partT")
        bounded(coefG, ref["coefG"], bnd["coefG"], f"{what} coefG")
        bounded(coefT, ref["coefT"], bnd["coefT"], f"{what} coefT")
    else:
        bounded(G, ref["partG"], bnd["partG"], f"{what} partG")
    bounded(loss, ref["loss"], bnd["loss"], f"{what} loss")
    unchanged({"logits": (xd, x)})
    assert torch.equal(td.cpu(), t)
    return ref, xd, td


def check_seg_bwd(shape, kind, mode, x, t, ref, xd, td, what):
    B, F, C, H, W = shape
    cG = R.round_to(ref["coefG"], F32) if mode == "tversky" else None
    cT = R.round_to(ref["coefT"], F32) if mode == "tversky" else None
    cGd, cTd = dev(cG), dev(cT)
    for dl in (None, -1.5):
        dld = None if dl is None else torch.tensor([dl], dtype=F32, device=DEV)
        dlogits = filled(shape)
        ops.seg_loss_bwd(xd, td, cGd, cTd, dld, dlogits, mode)
        sync()
        r = R.seg_loss_bwd(x, t, cG, cT, dl, mode)
        bounded(dlogits, r["dlogits"], R.seg_loss_bwd_bounds(r, shape, mode, kind, dl)["dlogits"], f"{what} dlogits, dloss {dl}")
    unchanged({"logits": (xd, x), "coefG": (cGd, cG), "coefT": (cTd, cT)})


@pytest.mark.parametrize("mode", R.SEG_MODES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SEG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_loss_fwd_bwd(shape, kind, mode):
    d = R.seg_data(shape, kind, mode)
    what = f"seg {mode} {kind}"
    ref, xd, td = check_seg_fwd(shape, kind, mode, d["logits"], d["target"], what)
    check_seg_bwd(shape, kind, mode, d["logits"], d["target"], ref, xd, td, what)


def test_seg_loss_fwd_with_other_weights_through_ops():
    shape = R.SEG_SHAPES[4]
    d = R.seg_data(shape, "continuous")
    cw, tw, al, be = R.SEG_OTHER
    ref = R.seg_loss_fwd(d["logits"], d["target"], "tversky", cw, tw, al, be)
    bnd = R.seg_loss_bounds(ref, shape, "tversky", "continuous", cw, tw, al, be)
    loss, coefG, coefT = ops.seg_loss_fwd(dev(d["logits"]), d["target"].to(DEV), "tversky", cw, tw, al, be)
    sync()
    bounded(loss, ref["loss"], bnd["loss"], "seg other weights loss")
    bounded(coefG, ref["coefG"], bnd["coefG"], "seg other weights coefG")
    C = shape[2]
    bounded(coefT[:, :, :C], ref["coefT"][:, :, :C], bnd["coefT"][:, :, :C], "seg other weights coefT")


def test_seg_loss_beyond_one_pass_of_the_grid():
    """more pixels than 16384 x 256: the grid-stride loop of seg_loss_bwd; 8 column blocks x 64 row splits in seg_loss_stats"""
    shape = R.SEG_BIG
    d = R.seg_data(shape, "continuous")
    ref, xd, td = check_seg_fwd(shape, "continuous", "tversky", d["logits"], d["target"], "seg grid-stride")
    B, F, C, H, W = shape
    cG, cT = R.round_to(ref["coefG"], F32), R.round_to(ref["coefT"], F32)
    dlogits = filled(shape)
    ops.seg_loss_bwd(xd, td, dev(cG), dev(cT), None, dlogits, "tversky")
    sync()
    r = R.seg_loss_bwd(d["logits"], d["target"], cG, cT, None, "tversky")
    bounded(dlogits, r["dlogits"], R.seg_loss_bwd_bounds(r, shape, "tversky", "continuous", None)["dlogits"], "seg grid-stride dlogits")


def test_seg_logf_error_is_within_the_constant():
    """-logf(p_t) of seg_loss_stats against float64 -log of the kernel's own float32 p_t, p_t over (0, 1); prints the worst error in
    units in the last place.  T_LOG_SEG is twice the figure this prints, rounded up to a whole unit."""
    d = R.seg_logf_data()
    F = R.SEG_LOGF_F
    loss, coefG, coefT, partG, partT = seg_launch(dev(d["logits"]), d["target"].to(DEV), "tversky")
    t = d["target"][0, :, 0, 0]
    p = partT.cpu().to(F64)[torch.arange(F), 0, 2, t, 0]
    nl = partG.cpu().to(F64)[torch.arange(F), 0, 2, t]
    want = -torch.log(p)
    assert (p > 0).all() and (p <= 1).all() and p.min() < 2.0 ** -20 and (p > 1 - 2.0 ** -20).any()
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want.abs().clamp_min(1e-300))[1] - 24)
    err = torch.where(want == 0, nl.abs() * 1e300, (nl - want).abs() / ulp)
    print(f"measured worst error of logf on (0, 1], units in the last place: {err.max().item():.3f}")
    assert err.max().item() <= R.T_LOG_SEG
