"""The contract the engines rely on (include/pmoe_hip.h, "what a non-negative plan means"): a descriptor with a fused request
runs on a kernel that implements it or on none, so ``plan >= 0`` answers "is the fusion applied" -- and the Python side asks
that question with the descriptor it launches and compares nothing with plan codes.  Planning calls only: no GPU."""
import ast
import ctypes as C
import itertools
from pathlib import Path

import pytest
import torch

from pmoe_amd import hip, ops
from pmoe_amd.hip import ConvDesc, WgradDesc

REPO = Path(__file__).resolve().parents[1]
BF, U8, F32 = torch.bfloat16, torch.uint8, torch.float32

# request -> the kernel instantiations that implement it (include/pmoe_hip.h).  This is where lists of codes belong.
IMPLEMENTED_BY = {
    "inbn_3x3": {1267},                                    # conv3x3_respipe_kernel<false, 3>
    "inbn_1x1": {1412, 1414},                              # conv1x1_direct_kernel<MT, true>
    "dbn": {1107, 1117, 1247, 1257, 5007, 5017},           # conv3x3_resdma_kernel, conv3x3_respipe_kernel<b, 2>, conv3x3_dma_kernel
    "shuffle_c": {1452, 1454},                             # conv1x1_direct_kernel<MT> with the scatter
    "shuffle_c+inbn": {1462, 1464},
    "in_fp8": {8507},                                      # conv3x3_dma_f8_kernel
    "wgrad_bn_fused": {7209},                              # conv_wgrad_bnbwd_kernel
}
SWITCHES = (None, "PMOE_RES_DMA", "PMOE_RES_PIPE", "PMOE_CONV_C1X1", "PMOE_CONV_DMA", "PMOE_CONV_F8DMA")      # all read per launch


def _conv(request, c, side, ipe, bias, stats, E=2):
    d = ConvDesc()
    ks = 3 if request in ("inbn_3x3", "dbn", "in_fp8") else 1
    shuf = c // 4 if request.startswith("shuffle_c") else 0
    d.n, d.h, d.w_, d.cin, d.ho, d.wo, d.cout, d.coutp = E * ipe, side, side, c, side, side, c, (c + 63) // 64 * 64
    d.in_ld, d.out_ld, d.out_coff, d.ipe, d.ks, d.stride, d.pad = c, 2 * shuf if shuf else c, shuf, ipe, ks, 1, ks // 2
    d.in_, d.w, d.out, d.shuffle_c = 1, 2, 3, shuf
    d.bias, d.stats = (7 if bias else None), (8 if stats else None)
    if "inbn" in request:
        d.res_mode, d.bn_coef = hip.RES_INBN, 5
    if request == "dbn":
        d.res_mode, d.res, d.res_ld, d.bn_coef = hip.RES_DBN, 4, c, 5
    if request == "in_fp8":
        d.w_fp8, d.in_fp8, d.in_scale, d.out_scale = 1, 1, 1.0, 6
    return d


def _wgrad(cin, cout, side, ipe, E=2):
    d = WgradDesc()
    d.n, d.h, d.w_, d.cin, d.cinp, d.ho, d.wo = E * ipe, side, side, cin, (cin + 63) // 64 * 64, side, side
    d.cout, d.coutp, d.x_ld, d.dy_ld, d.bn_z_ld = cout, (cout + 63) // 64 * 64, cin, cout, cout
    d.ipe, d.ks, d.stride, d.pad, d.per_image, d.bn_fused = ipe, 3, 1, 1, 1, 1
    return d


def test_a_fused_request_is_implemented_or_refused(monkeypatch):
    """Channels x map sides x images per expert x bias x statistics x the per-launch A/B switches, for every fused request: the
    plan is negative or one of the kernels that implement the request -- never a kernel that would drop it.
    pmoe_conv2d_stat_rows answers for the descriptor WITH statistics (its definition: include/pmoe_hip.h), so it is negative
    exactly when the plan of that descriptor is; the weight gradient's workspace query exactly when its plan is."""
    lib = hip.load()
    answers = {r: [0, 0] for r in IMPLEMENTED_BY}                 # [refused, served]
    grid = list(itertools.product((16, 64, 128, 256, 512), (8, 16, 32, 64, 128), (1, 2, 64)))
    for switch in SWITCHES:
        if switch:
            monkeypatch.setenv(switch, "0")
        for request, (c, side, ipe) in itertools.product(IMPLEMENTED_BY, grid):
            if request == "wgrad_bn_fused":
                for d in (_wgrad(16, c, side, ipe), _wgrad(c, 64, side, ipe)):
                    plan, ws = lib.pmoe_conv2d_wgrad_plan(C.byref(d)), lib.pmoe_conv2d_wgrad_ws_floats(C.byref(d))
                    assert plan < 0 or plan in IMPLEMENTED_BY[request], (switch, request, c, side, ipe, plan)
                    assert (ws < 0) == (plan < 0), (switch, request, c, side, ipe, plan, ws)
                    answers[request][plan >= 0] += 1
                continue
            for bias, stats in itertools.product((False, True), (False, True)):
                d = _conv(request, c, side, ipe, bias, stats)
                plan, rows = lib.pmoe_conv2d_plan(C.byref(d)), lib.pmoe_conv2d_stat_rows(C.byref(d))
                assert plan < 0 or plan in IMPLEMENTED_BY[request], (switch, request, c, side, ipe, bias, stats, plan)
                with_stats = plan if stats else lib.pmoe_conv2d_plan(C.byref(_conv(request, c, side, ipe, bias, True)))
                assert (rows < 0) == (with_stats < 0), (switch, request, c, side, ipe, bias, stats, plan, rows)
                if request.startswith("shuffle_c"):                 # (the scatter writes no statistics: that comparison is of two refusals)
                    assert rows == with_stats == hip.ERR_UNSUPPORTED and (not stats or plan < 0)
                answers[request][plan >= 0] += 1
        if switch:
            monkeypatch.delenv(switch)
    for request, (refused, served) in answers.items():          # the sweep asks every question both ways
        assert refused > 0 and served > 0, (request, refused, served)


def test_requests_no_kernel_combines_are_refused():
    """e4m3 activations without e4m3 weights, and a BatchNorm mode on e4m3 weights: the plan once named a kernel that ignores the
    request (the launch itself declined the first with PMOE_ERR_ARG and ran the second without the BatchNorm)."""
    lib = hip.load()
    d = _conv("in_fp8", 128, 64, 2, False, False)
    assert lib.pmoe_conv2d_plan(C.byref(d)) == 8507
    d.w_fp8 = 0
    assert lib.pmoe_conv2d_plan(C.byref(d)) == lib.pmoe_conv2d_stat_rows(C.byref(d)) == hip.ERR_UNSUPPORTED
    for request in ("inbn_3x3", "inbn_1x1", "dbn"):
        d = _conv(request, 64, 128, 2, False, True)
        assert lib.pmoe_conv2d_plan(C.byref(d)) in IMPLEMENTED_BY[request]
        d.w_fp8, d.in_scale, d.out_scale = 1, 1.0, 6
        assert lib.pmoe_conv2d_plan(C.byref(d)) == lib.pmoe_conv2d_stat_rows(C.byref(d)) == hip.ERR_UNSUPPORTED, request


def _t(*shape, dtype=BF):
    return torch.empty(*shape, dtype=dtype, device="meta")           # shapes and dtypes only


ONE_DESCRIPTOR_CASES = {
    # name: (x, w, out, conv2d keywords that are tensors, the other conv2d keywords, planning-only keywords)
    "3x3 + bias + statistics": (_t(8, 32, 32, 64), _t(2 * 64 * 9 * 64), _t(8, 32, 32, 64), dict(bias=_t(2, 64, dtype=F32), stats=True),
                                dict(cin=64, cout=64, coutp=64, ipe=4, ks=3, stride=1, pad=1, act=hip.ACT_RELU), {}),
    "windows of wider buffers": (_t(8, 32, 32, 256), _t(2 * 128 * 9 * 64), _t(8, 16, 16, 384), {},
                                 dict(cin=64, cout=128, coutp=128, ipe=4, ks=3, stride=2, pad=1, in_coff=64, out_coff=128, drop_p=0.25,
                                      seed=77), {}),
    "ConvTranspose2d scatter (shuffle2_c)": (_t(4, 64, 64, 128), _t(2 * 256 * 128), _t(4, 128, 128, 128), dict(bias=_t(2, 256, dtype=F32)),
                                             dict(cin=128, cout=256, coutp=256, ipe=2, ks=1, stride=1, pad=0, out_coff=64, shuffle2_c=64), {}),
    "BatchNorm + ReLU on load": (_t(4, 128, 128, 64), _t(2 * 64 * 9 * 64), _t(4, 128, 128, 64), dict(bn_coef=_t(4, 2, 64, dtype=F32), stats=True),
                                 dict(cin=64, cout=64, coutp=64, ipe=2, ks=3, stride=1, pad=1, res_mode=hip.RES_INBN), {}),
    "BatchNorm backward in the data gradient": (_t(4, 64, 64, 128), _t(2 * 128 * 9 * 128), _t(4, 64, 64, 128),
                                                dict(res=_t(4, 64, 64, 128), bn_coef=_t(4, 2, 128, dtype=F32), stats=True),
                                                dict(cin=128, cout=128, coutp=128, ipe=2, ks=3, stride=1, pad=1, res_mode=hip.RES_DBN, bn_ipe=2), {}),
    "shared input, stride-2 data gradient": (_t(4, 16, 16, 128), _t(2 * 64 * 9 * 128), _t(8, 32, 32, 64), dict(res=_t(8, 32, 32, 64)),
                                             dict(cin=128, cout=64, coutp=64, ipe=4, ks=3, stride=1, pad=1, dilate=True, in_shared=True,
                                                  res_mode=hip.RES_DRELU, drop_p=0.5), {}),
    "e4m3 weights and activations": (_t(4, 64, 64, 128, dtype=U8), _t(2 * 128 * 9 * 128, dtype=U8), _t(4, 64, 64, 128),
                                     dict(out_scale=_t(2, 128, dtype=F32), stats=True),
                                     dict(cin=128, cout=128, coutp=128, ipe=2, ks=3, stride=1, pad=1, in_scale=0.5), dict(w_fp8=True, in_fp8=True)),
}


@pytest.mark.parametrize("case", list(ONE_DESCRIPTOR_CASES))
def test_the_prepared_launch_and_the_planning_call_build_one_descriptor(case):
    """ops.conv2d_prepare (what launches) against ops._planning_desc (what conv2d_plan / conv2d_stat_rows ask) from the same
    shapes and keywords: every non-pointer field equal, every pointer field null in both or in neither -- and so the same answers."""
    x, w, out, tensors, kw, plan_kw = ONE_DESCRIPTOR_CASES[case]
    kw = dict(kw)
    run = ops.conv2d_prepare(x, w, out, shapes_only=True, **tensors, **kw)
    ho, wo = (out.shape[1] // 2, out.shape[2] // 2) if kw.get("shuffle2_c") else out.shape[1:3]
    geom = {k: kw.pop(k) for k in ("cin", "cout", "coutp", "ipe", "ks", "stride", "pad")}
    res = tensors.get("res")
    d = ops._planning_desc(out.shape[0], x.shape[1], x.shape[2], ho, wo, *geom.values(), BF, bias="bias" in tensors, stats="stats" in tensors,
                           in_ld=x.shape[-1], out_ld=out.shape[-1], res_ld=res.shape[-1] if res is not None else 0, **kw, **plan_kw)
    for name, ctype in ConvDesc._fields_:
        a, b = getattr(run.d, name), getattr(d, name)
        assert (bool(a) == bool(b)) if ctype is C.c_void_p else (a == b), (name, a, b)
    assert run.plan() == hip.load().pmoe_conv2d_plan(C.byref(d))
    assert hip.load().pmoe_conv2d_stat_rows(C.byref(run.d)) == hip.load().pmoe_conv2d_stat_rows(C.byref(d))
    with pytest.raises(ValueError, match="shapes only"):
        run.launch()


def test_the_wgrad_queries_say_what_plan_only_said():
    """conv2d_wgrad_bn_served / conv2d_wgrad_nsplit from shapes = the two meanings ``conv2d_wgrad(plan_only=True)`` has."""
    lib = hip.load()
    geom = (2 * 4, 128, 128, 128, 128, 16, 64, 64, 64, 4, 3, 1, 1)
    assert ops.conv2d_wgrad_bn_served(*geom, BF, x_shared=True, per_image=True) is True
    assert ops.conv2d_wgrad_bn_served(*geom, F32, x_shared=True, per_image=True) is False
    assert ops.conv2d_wgrad_bn_served(*geom, BF, x_shared=True) is False                      # not per image
    for n, side, c, ipe in ((8, 64, 64, 4), (128, 32, 256, 64), (2, 16, 128, 1)):
        d = ops._wgrad_desc(n, side, side, side, side, c, c, c, c, ipe, 3, 1, 1, hip.DT_BF16)
        need = lib.pmoe_conv2d_wgrad_ws_floats(C.byref(d))
        assert ops.conv2d_wgrad_nsplit(n, side, side, side, side, c, c, c, c, ipe, 3, 1, 1, BF) == max(1, need // ((n // ipe) * 9 * c * c))


def test_the_engines_compare_nothing_with_plan_codes():
    """pmoe_amd/engine.py and engine_punet.py: no comparison has an integer literal >= 1000 (a plan code), or a tuple of such, on
    either side -- which kernel serves a launch is the library's knowledge (the 1536-wide feature slices are no comparisons)."""
    def codes(node):
        if isinstance(node, ast.Constant):
            return type(node.value) is int and node.value >= 1000
        return isinstance(node, (ast.Tuple, ast.List, ast.Set)) and any(codes(e) for e in node.elts)
    for name in ("engine.py", "engine_punet.py"):
        tree = ast.parse((REPO / "pmoe_amd" / name).read_text())
        bad = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Compare) and any(codes(s) for s in [n.left] + n.comparators)]
        assert not bad, (name, bad)
