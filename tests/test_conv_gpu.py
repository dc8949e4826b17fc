"""Every convolution kernel (csrc/conv_igemm.hip, conv_dma.hip + conv_dma_epilogue.inc, conv_res.hip, conv_c1x1.hip,
conv_c16.hip, gemm_skinny.hip, conv_wgrad.hip), pmoe_mlp_wgrad and the weight packs against the float64 reference of their own
operation (tests/conv_ref.py), at the smallest shapes that reach each plan code (conv_ref.CASES; tests/test_conv_cpu.py proves
that the table covers every code the planners answer), through pmoe_amd.ops, the binding the engines use.

Four kinds of input (tests/test_conv_cpu.py checks on the CPU what is assumed of them here):
  lattice  integers with sum |x||w| < 2^24: a float32 accumulation is exact in any order, so every STORED element must equal the
           reference's, rounded in the order conv_ref.ROUNDING names for the kernel -- one missing or doubled term, a truncation, a
           second rounding or a residual left out all show as unequal elements.  Fused statistics: per-expert totals within
           (L + 8) 2^-24 sum|term|, L = conv_ref.chain_stats.
  unit     {-1, 0, 1}: nothing rounds and the statistics are exact too.
  dyadic   the cases with an MLP epilogue form (ELU / tanh / sigmoid, their derivatives from the saved output, fused dropout), in
           all three copies of that epilogue: the accumulator is exact, the pre-activations are spread over (-8, 8).  Where the
           reference's allowance is zero -- no activation, ReLU, ELU's positive branch, every dropout product, every derivative
           chain that float32 evaluates without a rounding -- the stored element must EQUAL the reference's; elsewhere it lies
           in [round(ref - allow), round(ref + allow)], which is one value for all but a per cent of the elements.  The dropout
           mask is compared element for element with the hash wherever the undropped value is non-zero.
           Continuous data stays in tests/test_ops_gpu.py for the K-long float32 sums only.
  select   the cases with e4m3 operands, next to lattice and unit (both fixed points of the e4m3 quantisers, so the reference is
           unchanged and equality holds): one non-zero weight +-2^j per output channel, inputs that hold every e4m3 value, tie,
           underflow and overflow (bfloat16 input) or all 254 non-NaN byte codes (e4m3 input) -- every stored element equals
           +-2^j times the policy's conversion of one input element, whatever the loader, chunk width and tap.  The operands of
           such a launch (weight bytes, out_scale with NaN past cout, input bytes with 0x7f outside the window) come from
           conv_ref.e4m3_operands, the reference's own statement.
Every buffer is compared WHOLE: outputs are sentinel-filled before the launch, so pad channels, the other columns of out_ld, the
untouched half of a concatenation buffer and the odd pixels of the in-place stride-2 1x1 gradient must come back unchanged;
everything outside an input's channel window is NaN, so a read outside it poisons the output.  The plan code is asserted before
each launch; every kernel gets the generator's (= the reference's) inputs, never another kernel's output.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests import conv_ref as R  # noqa: E402
from tests.test_bn_gpu import same  # noqa: E402
from tests.test_conv_cpu import case_kinds, conv_prepare, conv_tensors, set_switches, wgrad_plan  # noqa: E402

DEV = "cuda"
F64, F32, BF16 = R.F64, R.F32, R.BF16
EPS = R.EPS24
CONV_CASES = [c for c in R.CASES if c.codes[0] is not None or c.codes[1] is not None]
WGRAD_CASES = [c for c in R.CASES if c.codes[2] is not None]


def ids(cases):
    return [R.case_id(c) for c in cases]


def check_conv_launch(L, code_expected, kind, what):
    kw = L["kw"]
    t = conv_tensors(L, DEV)
    p = conv_prepare(L, t)
    code = p.plan()
    assert code == code_expected, f"{what}: routed to kernel code {code}, this case is meant for {code_expected}"
    E, cout, coutp = L["w"].shape[0], kw["cout"], R.r64(kw["cout"])
    guard = None
    if kw["stats"]:
        rows = p.stat_rows()
        assert rows > 0 and rows % E == 0, (rows, E)
        guard = torch.full((rows + 3, 2, coutp), float("nan"), dtype=F32, device=DEV)
        p = conv_prepare(L, t, stats=guard[:rows])
    p.launch()
    torch.cuda.synchronize()
    order = R.rounding_of(code, kw.get("res_mode", R.RES_NONE), L["bias"] is not None, kw.get("act", R.ACT_NONE))
    ref = R.conv_reference(L, order)
    got = t["out"].cpu().to(F64)
    if kind == R.DYADIC:
        check_mlp_forms(got, ref, L, code, what)
    elif not (got == ref["out"]).all():
        other = R.conv_reference(L, "staged" if order == "once" else "once")["out"]
        hint = f" (it DOES equal the '{'staged' if order == 'once' else 'once'}' order)" if (got == other).all() else ""
        same(got, ref["out"], f"{what}: code {code}, rounding order '{order}'{hint}")
    if kw.get("res_mode", R.RES_NONE) not in (R.RES_DRELU, R.RES_DELU, R.RES_DTANH, R.RES_DSIGMOID, R.RES_DBN):
        # the sign of a zero is exempt in MASKED gradients only (+0 or -0 by how the mask is applied): bit for bit elsewhere
        neg = torch.signbit(t["out"].float().cpu()) != torch.signbit(ref["out"].to(F32))
        assert not neg.any(), f"{what}: code {code}: {int(neg.sum())} elements differ in sign only (a zero of the other sign); first {neg.nonzero()[:4].tolist()}"
    for name, src in (("x", L["inp"]), ("res", None if L["res_is_out"] else L["res"])):
        if src is not None and t[name].dtype == torch.uint8:           # (e4m3 input bytes: 0x7f outside the window)
            assert torch.equal(t[name].cpu(), R.e4m3_operands(L, coutp)[2]), f"{what}: {name} modified"
        elif src is not None:                                          # inputs come back as they went in (NaN outside the windows)
            back = t[name].cpu().to(F64)
            assert torch.equal(torch.isnan(back), torch.isnan(src)) and torch.equal(back.nan_to_num(), src.nan_to_num()), f"{what}: {name} modified"
    if guard is None:
        return
    g = guard.cpu().to(F64)
    assert torch.isnan(g[rows:]).all(), f"{what}: statistics rows beyond conv2d_stat_rows = {rows} written"
    assert not torch.isnan(g[:rows, :, :cout]).any(), f"{what}: statistics rows left unwritten"
    tot = g[:rows].reshape(E, rows // E, 2, coutp).sum(1)[..., :cout]
    n, ho, wo = ref["acc"].shape[:3]
    Lc = R.chain_stats(code, R.tiles_per_expert(code, kw["ipe"], ho, wo), rows // E)
    err = (tot - ref["sums"]).abs()
    print(f"{what}: statistics rows {rows}, L {Lc}, max err / (2^-24 sum|term|) "
          f"{(err / (EPS * ref['sums_abs']).clamp_min(1e-300)).max().item():.2f}")
    if kind == "unit":
        same(tot, ref["sums"], f"{what}: statistics totals (exact on the unit kind)")
    else:
        bad = err > (Lc + 8) * EPS * ref["sums_abs"]
        assert not bad.any(), (f"{what}: {int(bad.sum())} statistics totals beyond (L + 8) 2^-24 sum|term|, L = {Lc}; first "
                               f"{bad.nonzero()[:4].tolist()}, worst err {err.max().item():.3e}")


def check_mlp_forms(got, ref, L, code, what):
    """a launch with an MLP epilogue form: the window within the reference's interval of stored values (equal where the allowance
    is zero), the dropout mask equal to the hash mask, everything outside the window untouched"""
    kw = L["kw"]
    dtype, c0, c1 = kw["dtype"], kw["out_coff"], kw["out_coff"] + kw["cout"]
    outside = torch.ones(got.shape[-1], dtype=torch.bool)
    outside[c0:c1] = False
    same(got[..., outside], ref["out"][..., outside], f"{what}: code {code}: channels outside the output window")
    win = got[..., c0:c1]
    assert not torch.isnan(win).any(), f"{what}: code {code}: NaN in the output window (a read outside an input window?)"
    if kw.get("drop_p", 0.0) > 0 and kw.get("res_mode", R.RES_NONE) < R.RES_DRELU:
        seen = ref["undropped"] != 0
        wrong = ((win != 0) != ref["keep"]) & seen
        assert not wrong.any(), (f"{what}: code {code}: the dropout mask differs from hash_uniform(seed, opix * Cout + c) >= p in "
                                 f"{int(wrong.sum())} elements; first {wrong.nonzero()[:4].tolist()}")
    lo, hi = R.stored_interval(ref, dtype)
    exact = ref["allow"] == 0
    bad = (win < lo) | (win > hi)
    nz = ref["stored"] != 0
    off = (win - ref["pre"]).abs()
    if dtype == BF16:
        # the least error of the float32 value that explains the stored bfloat16: its distance to the reference beyond half a step
        off_f32 = (off - torch.ldexp(torch.ones_like(win), torch.frexp(win)[1] - 9)).clamp_min(0)
    else:
        off_f32 = off
    ratio = (off_f32[~exact] / ref["allow"][~exact]).max().item() if (~exact).any() else 0.0
    print(f"{what}: code {code}: {int(exact.sum())} of {exact.numel()} elements exact (all equal: {bool((win == ref['stored'])[exact].all())}); "
          f"{int(((lo != hi) & nz).sum())} open between two stored values, {int(((win != ref['stored']) & ~bad).sum())} of them on the "
          f"neighbour of the rounded reference; worst error of the float32 value / allowance {ratio:.3f}; "
          f"worst |got - ref| / |ref| {(off / ref['pre'].abs().clamp_min(1e-30))[nz].max().item() if nz.any() else 0.0:.3e}")
    if bad.any():
        i = bad.nonzero()[:6]
        rows = [(tuple(j.tolist()), win[tuple(j)].item(), lo[tuple(j)].item(), hi[tuple(j)].item(), ref["allow"][tuple(j)].item()) for j in i]
        raise AssertionError(f"{what}: code {code}: {int(bad.sum())} of {bad.numel()} elements outside [round(ref - allow), round(ref + allow)] "
                             f"({int((bad & exact).sum())} of them where the allowance is zero); first (index, got, lo, hi, allow): {rows}")


@pytest.mark.parametrize(**case_kinds(CONV_CASES))
def test_conv_launches_match_reference(case, kind, monkeypatch):
    """forward and data gradient of the case, each under its request: stored output, untouched bytes, statistics"""
    set_switches(monkeypatch, case)
    ls = R.launches(case, kind)
    for i, k in enumerate("fd"):
        if k in ls:
            check_conv_launch(ls[k], case.codes[i], kind, f"{'forward' if k == 'f' else 'data gradient'} [{R.flags(case)[k] and '+'.join(sorted(R.flags(case)[k]))}]")


SENTINEL = R.SENTINEL


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=ids(WGRAD_CASES))
def test_wgrad_matches_reference(case, kind, monkeypatch):
    """dw_ws exact with its pad rows and columns (zeros: every element is stored); the parameter-layout gradient of the fused
    fold, of the deferred fold and of pmoe_unpack_conv_wgrad bit-identical to each other and to the reference"""
    set_switches(monkeypatch, case)
    L = R.launches(case, kind)["w"]
    kw = L["kw"]
    dtype = kw["dtype"]
    code, nsplit = wgrad_plan(L)
    assert code == case.codes[2], f"weight gradient routed to kernel code {code}, this case is meant for {case.codes[2]}"
    ref = R.wgrad_reference(L)
    x, dy = L["x"].to(dtype).to(DEV), L["dy"].to(dtype).to(DEV)
    bn = None
    if L["bn"] is not None:
        z, coef, c1, c2 = L["bn"]
        bn = (z.to(dtype).to(DEV), coef.to(F32).to(DEV), c1.to(F32).to(DEV), c2.to(F32).to(DEV))
    common = dict(cin=kw["cin"], cout=kw["cout"], cinp=kw["cinp"], coutp=kw["coutp"], ipe=kw["ipe"], ks=kw["ks"], stride=kw["stride"],
                  pad=kw["pad"], x_shared=kw["x_shared"], x_coff=kw["x_coff"], dy_coff=kw["dy_coff"], per_image=kw["per_image"], bn_fuse=bn)
    ws = torch.full(ref["dw_ws"].shape, SENTINEL, dtype=F32, device=DEV)
    ops.conv2d_wgrad(x, dy, ws, **common)
    torch.cuda.synchronize()
    print(f"weight gradient: code {code}, K-split {nsplit}, workspace {tuple(ws.shape)}")
    same(ws, ref["dw_ws"], f"dw_ws (code {code}, K-split {nsplit})")
    for name, t, src in (("x", x, L["x"]), ("dy", dy, L["dy"])):
        assert torch.equal(t.cpu().to(F64).nan_to_num(), src.nan_to_num()), f"{name} modified"
    if kw["per_image"]:
        return
    E, cout, cin, ks = ws.shape[0], kw["cout"], kw["cin"], kw["ks"]
    shape = (E, cout, cin, ks, ks)
    fused, deferred, unpacked = (torch.full(shape, SENTINEL, dtype=F32, device=DEV) for _ in range(3))
    scratch = torch.full_like(ws, SENTINEL)
    ops.conv2d_wgrad(x, dy, scratch, grads=fused.view(-1), grads_cout=cout, grads_cin=cin, **common)
    d = ops.conv2d_wgrad(x, dy, scratch, grads=deferred.view(-1), grads_cout=cout, grads_cin=cin, defer_fold=True, **common)
    ops.conv2d_wgrad_fold(d)
    ops.unpack_conv_wgrad(ref["dw_ws"].to(F32).to(DEV), unpacked, E, cout, cin, ks, kw["coutp"], kw["cinp"])
    torch.cuda.synchronize()
    same(fused, ref["grads"], "grads of the fused fold")
    same(deferred, ref["grads"], "grads of the deferred fold")
    same(unpacked, ref["grads"], "pmoe_unpack_conv_wgrad of the reference's workspace")
    assert torch.equal(fused, deferred) and torch.equal(fused, unpacked)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 3, 24, 12, 3), (3, 2, 72, 40, 1), (1, 2, 64, 64, 3)], ids=lambda s: "x".join(map(str, s)))
def test_weight_packs_match_reference(shape, dtype):
    """forward, data-gradient (taps reversed), scaled and gated packs on lattice values whose products are exact: every element,
    pad rows and columns zero"""
    E, ipe, cout, cin, ks = shape
    g = torch.Generator().manual_seed(sum(shape))
    coutp, cinp, cinp2, coutp2 = R.r64(cout), R.r16(cin), R.r64(cin), R.r16(cout)
    w = torch.randint(-7, 8, (E, cout, cin, ks, ks), generator=g).to(F64)
    dev_w = [w[e].to(F32).to(DEV).contiguous() for e in range(E)]
    tab = hip.ptr_table(dev_w, DEV)
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=DEV)
    fwd, dgrd = nan(E, coutp, ks * ks, cinp), nan(E, cinp2, ks * ks, coutp2)
    ops.pack_conv_weights(tab, fwd, dgrd, E, cout, cin, ks, coutp, cinp, cinp2, coutp2, dtype)
    rf, rd = R.pack_weights(w, coutp, cinp, dtype, cinp2, coutp2)
    same(fwd, rf, "forward pack")
    same(dgrd, rd, "data-gradient pack")
    # eval-mode BatchNorm folded in: W * scale (integers and halves up to 21: exact in bfloat16), bias = shift - mean * scale
    pick = lambda vals, *s: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), s, generator=g)]
    scale, shift, mean = pick([-2.0, -1.0, 0.5, 1.0, 2.0, 3.0], E, cout), pick([-1.5, -0.5, 0.0, 0.25, 2.0], E, cout), pick([-0.75, 0.0, 0.5, 1.25], E, cout)
    fs, bias = nan(E, coutp, ks * ks, cinp), torch.full((E, coutp), float("nan"), dtype=F32, device=DEV)
    ops.pack_conv_weights_scaled(tab, scale.to(F32).to(DEV), shift.to(F32).to(DEV), mean.to(F32).to(DEV), fs, bias, E, cout, cin, ks,
                                 coutp, cinp, dtype)
    rs, rb = R.pack_weights_scaled(w, scale, shift, mean, coutp, cinp, dtype)
    same(fs, rs, "scaled pack")
    same(bias, rb, "bias of the scaled pack")
    # per-image packs with the ECA gate folded in
    N, gate_ld = E * ipe, R.r16(cin) + 16
    gate = pick([0.0, 0.25, 0.5, 1.0, 2.0], N, gate_ld)
    fg, dg = nan(N, coutp, ks * ks, cinp), nan(N, cinp2, ks * ks, coutp2)
    ops.pack_conv_weights_gated(tab, gate.to(F32).to(DEV), fg, dg, N, ipe, cout, cin, ks, coutp, cinp, cinp2, coutp2, dtype)
    rg, rgd = R.pack_weights_gated(w, gate, ipe, coutp, cinp, dtype, cinp2, coutp2)
    same(fg, rg, "gated forward pack")
    same(dg, rgd, "gated data-gradient pack")
    # and back: workspace -> parameter layout
    ckw = 64 if dtype == BF16 else 32
    cop, cip = (cout + ckw - 1) // ckw * ckw, (cin + ckw - 1) // ckw * ckw
    ws = torch.randint(-999, 1000, (E, ks * ks, cop, cip), generator=g).to(F64)
    grads = torch.full((E, cout, cin, ks, ks), float("nan"), dtype=F32, device=DEV)
    ops.unpack_conv_wgrad(ws.to(F32).to(DEV), grads, E, cout, cin, ks, cop, cip)
    torch.cuda.synchronize()
    same(grads, R.unpack_wgrad(ws, cout, cin, ks), "pmoe_unpack_conv_wgrad")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.MLP_WGRAD_CASES, ids=["-".join(str(int(v)) for v in c) for c in R.MLP_WGRAD_CASES])
def test_mlp_wgrad_matches_reference(case, kind):
    """pmoe_mlp_wgrad with and without bias_grads: both outputs exact and whole (sentinels around them: the pad channels staged
    with 2^60, the NaN outside the channel windows and the rows of the next expert reach nothing), grads bit-identical between
    the two launches, inputs unmodified"""
    E, ipe, cin, cin_real, cout, cout_real, shared, xc, dc = case
    d = R.mlp_wgrad_data(case, kind)
    ref = R.mlp_wgrad(d["x"], d["dy"], **d["kw"])
    x = d["x"].to(BF16).to(DEV).reshape(-1, 1, 1, d["x"].shape[1])
    dy = d["dy"].to(BF16).to(DEV).reshape(-1, 1, 1, d["dy"].shape[1])
    ng, nb = E * cout_real * cin_real, E * cout_real
    runs = []
    for with_bias in (True, False):
        gbuf = torch.full((ng + R.GUARD,), SENTINEL, dtype=F32, device=DEV)
        bbuf = torch.full((nb + R.GUARD,), SENTINEL, dtype=F32, device=DEV)
        ops.mlp_wgrad(x, dy, gbuf[:ng], bbuf[:nb] if with_bias else None, **d["kw"])
        torch.cuda.synchronize()
        want_g = torch.cat([ref["grads"].flatten(), torch.full((R.GUARD,), SENTINEL, dtype=F64)])
        want_b = torch.cat([ref["bias_grads"].flatten() if with_bias else torch.full((nb,), SENTINEL, dtype=F64),
                            torch.full((R.GUARD,), SENTINEL, dtype=F64)])
        same(gbuf, want_g, f"grads with its guard (bias_grads {'set' if with_bias else 'null'})")
        same(bbuf, want_b, f"bias_grads with its guard (bias_grads {'set' if with_bias else 'null'})")
        runs.append(gbuf)
    assert torch.equal(runs[0], runs[1]), "grads differ between the launches with and without bias_grads"
    for name, t, src in (("x", x, d["x"]), ("dy", dy, d["dy"])):
        back = t.cpu().to(F64).reshape(src.shape)
        assert torch.equal(torch.isnan(back), torch.isnan(src)) and torch.equal(back.nan_to_num(), src.nan_to_num()), f"{name} modified"
    print(f"mlp_wgrad {case} {kind}: grads {tuple(ref['grads'].shape)} and bias_grads exact, max |grad| {ref['grads'].abs().max().item():.0f}")
