"""The float64 convolution reference (tests/conv_ref.py) checked against float64 torch.autograd of F.conv2d / F.conv_transpose2d /
F.batch_norm, its input generators checked for everything tests/test_conv_gpu.py assumes of them, and the case table checked
against the planners: every case plans to the codes it names, and every code the planners can answer over a grid of shapes,
requests and switches -- e4m3 operands among them -- is in the table: there is no exclusion list.  The same for the MLP epilogue
forms (activations, their derivatives from the saved output, fused dropout: conv_ref.mlp_epilogue on the dyadic kind, with a
case for every copy of that epilogue the planner reaches), for the operands of the e4m3 launches (the lattice and unit kinds are
fixed points of the quantisers of oracle/fp8_policy.py; the select kind) and for pmoe_mlp_wgrad with every refusal of its entry
point; and the proof that the inputs discriminate: each deliberately wrong variant of the reference is told apart by some case.
No GPU: pmoe_conv2d_plan and pmoe_conv2d_wgrad_plan are host code, and a refused call launches nothing."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from pmoe_amd import hip, ops
from tests import bn_ref
from tests import conv_ref as R
from tests import eca_head_ref as H
from tests.stem_tail_ref import bf16_boundary_distance

F64, F32, BF16 = R.F64, R.F32, R.BF16
IDS = [R.case_id(c) for c in R.CASES]


# ---------------------------------------------------------------------------------------------------------------------------------
# a launch of conv_ref.launches as ops sees it (tests/test_conv_gpu.py runs the same objects)

def conv_tensors(L, device):
    """the tensors of a conv launch in their storage types: on ``device``, or -- device "meta" -- shapes and types only"""
    kw = L["kw"]
    dtype, E, ks = kw["dtype"], L["w"].shape[0], kw["ks"]
    coutp = R.r64(kw["cout"])
    f8, a8 = L.get("f8", False), L.get("a8", False)
    x8 = oscale = None
    if device == "meta":
        mk = lambda t, dt: None if t is None else torch.empty(t.shape, dtype=dt, device="meta")
        wp = torch.empty(E, coutp, ks * ks, kw["cin"], dtype=torch.uint8 if f8 else dtype, device="meta")
        bias = None if L["bias"] is None else torch.empty(E, coutp, dtype=F32, device="meta")
        if f8:
            oscale, x8 = torch.empty(E, coutp, dtype=F32, device="meta"), mk(L["inp"], torch.uint8) if a8 else None
    else:
        mk = lambda t, dt: None if t is None else t.to(dt).to(device).contiguous()
        if f8:
            # e4m3 operands, built from the reference's statement (conv_ref.e4m3_operands), never by another kernel
            wp, oscale, x8 = (None if v is None else v.to(device).contiguous() for v in R.e4m3_operands(L, coutp))
        else:
            wp = mk(R.pack_weights(L["w"], coutp, kw["cin"], dtype), dtype)
        bias = None
        if L["bias"] is not None:
            bias = torch.zeros(E, coutp, dtype=F32)
            bias[:, :kw["cout"]] = L["bias"].to(F32)
            bias = bias.to(device)
    t = {"x": x8 if a8 else mk(L["inp"], dtype), "w": wp, "out": mk(L["out_init"], dtype), "bias": bias,
         "bn_coef": mk(L["bn_coef"], F32), "out_scale": oscale}
    t["res"] = t["out"] if L["res_is_out"] else mk(L["res"], dtype)
    return t


def conv_prepare(L, t, stats=None):
    """ops.conv2d_prepare of the launch on the tensors ``t``"""
    kw = L["kw"]
    return ops.conv2d_prepare(
        t["x"], t["w"], t["out"], cin=kw["cin"], cout=kw["cout"], coutp=R.r64(kw["cout"]), ipe=kw["ipe"], ks=kw["ks"],
        stride=kw["stride"], pad=kw["pad"], dilate=kw.get("dilate", False), in_shared=kw.get("in_shared", False),
        in_coff=kw["in_coff"], out_coff=kw["out_coff"], res=t["res"], res_coff=kw.get("res_coff", 0),
        res_mode=kw.get("res_mode", hip.RES_NONE), bias=t["bias"], act=kw.get("act", hip.ACT_NONE),
        drop_p=kw.get("drop_p", 0.0), seed=kw.get("seed", 0), stats=(True if stats is None else stats) if kw["stats"] else None,
        bn_coef=t["bn_coef"], bn_ipe=kw.get("bn_ipe", 0), shuffle2_c=kw.get("shuffle_c", 0), out_scale=t["out_scale"],
        in_scale=L.get("in_scale", 1.0), shapes_only=t["x"].device.type == "meta")


def wgrad_desc(L):
    """the pmoe_wgrad_desc of a weight-gradient launch, pointers null: what the planning calls read"""
    kw = L["kw"]
    n, ho, wo, dy_ld = L["dy"].shape
    _, h, w_, x_ld = L["x"].shape
    return ops._wgrad_desc(n, h, w_, ho, wo, kw["cin"], kw["cout"], kw["cinp"], kw["coutp"], kw["ipe"], kw["ks"], kw["stride"],
                           kw["pad"], hip._TORCH_DT[kw["dtype"]], x_ld=x_ld, dy_ld=dy_ld, x_coff=kw["x_coff"], dy_coff=kw["dy_coff"],
                           x_shared=kw["x_shared"], per_image=kw["per_image"], bn_z_ld=None if L["bn"] is None else L["bn"][0].shape[-1])


def wgrad_plan(L):
    """(plan code, K-split count)"""
    d = wgrad_desc(L)
    code = hip.load().pmoe_conv2d_wgrad_plan(C.byref(d))
    return code, (ops._wgrad_ws(d)[1] if code >= 0 else 0)


def set_switches(monkeypatch, case):
    for k, v in case.switches:
        monkeypatch.setenv(k, v)


def planned_codes(case):
    ls = R.launches(case, R.kinds_of(case)[-1])
    conv = lambda k: conv_prepare(ls[k], conv_tensors(ls[k], "meta")).plan() if k in ls else None
    return conv("f"), conv("d"), wgrad_plan(ls["w"])[0] if "w" in ls else None


# ---------------------------------------------------------------------------------------------------------------------------------
# routing and coverage

@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_case_plans_to_the_codes_it_names(case, monkeypatch):
    set_switches(monkeypatch, case)
    assert planned_codes(case) == case.codes


CHANNELS = (16, 32, 48, 64, 128, 192, 256, 512)
SIDES = (4, 7, 8, 16, 32, 64, 128)
IPES = (1, 2, 5)
# every switch conv_select / wgrad_select read per launch (csrc: sw("PMOE_...")), at the value that turns its kernel off; the
# tri-state ones also at their "always" value
CONV_SWITCHES = (None, ("PMOE_CONV_C16", "0"), ("PMOE_RES_DMA", "0"), ("PMOE_RES_PIPE", "0"), ("PMOE_CONV_C1X1", "0"),
                 ("PMOE_CONV_DMA", "0"), ("PMOE_DMA_STREAM", "0"), ("PMOE_DMA_STREAM", "2"), ("PMOE_DMA_PRODUCER", "0"),
                 ("PMOE_DMA_PRODUCER", "2"), ("PMOE_DMA_NARROW", "0"), ("PMOE_DMA_MF16", "0"), ("PMOE_DMA_MF16", "1"),
                 ("PMOE_CONV_F8DMA", "0"))
# the second, narrow sweep (no switch): many images per expert on small maps -- >= 4096 pixels per expert where neither the
# LDS-DMA kernels nor the LITE tile fit (742 | 4742 | 8742) -- and 8-channel layers (float32 522 | 541 as plain launches)
SMALL_SIDES = (2, 4, 8)
MANY_IPES = (64, 256)
CHANNELS_8 = (8,) + CHANNELS
WGRAD_SWITCHES = (None, ("PMOE_WGRAD_DMA", "0"), ("PMOE_WGRAD_NARROW", "0"), ("PMOE_WGRAD_V2", "0"), ("PMOE_WGRAD_REQ", "0"),
                  ("PMOE_WGRAD_REQ", "2"), ("PMOE_WGRAD_PIPE", "0"))
# request -> (keywords of ops._planning_desc, the launch is a data gradient, res == out)
REQUESTS = {
    "plain": ({}, False), "bias": (dict(bias=True), False), "stats": (dict(stats=True), False),
    "bias+relu": (dict(bias=True, act=hip.ACT_RELU), False), "add": (dict(res_mode=hip.RES_ADD), False),
    "add+stats": (dict(res_mode=hip.RES_ADD, stats=True), False), "drelu": (dict(res_mode=hip.RES_DRELU), False),
    "dbn": (dict(res_mode=hip.RES_DBN, stats=True), False), "dbn+bias": (dict(res_mode=hip.RES_DBN, stats=True, bias=True), False),
    "inbn": (dict(res_mode=hip.RES_INBN), False), "inbn+stats": (dict(res_mode=hip.RES_INBN, stats=True), False),
    "inbn+bias": (dict(res_mode=hip.RES_INBN, bias=True), False), "shared": (dict(in_shared=True), False),
    "shuffle": ("shuffle", False), "shuffle+inbn": ("shuffle+inbn", False),
    "dgrad": ({}, True), "dgrad+bias": (dict(bias=True), True), "dgrad+add": (dict(res_mode=hip.RES_ADD), True),
    "dgrad+addin": (dict(res_mode=hip.RES_ADD), True), "dgrad+drelu": (dict(res_mode=hip.RES_DRELU), True),
    "dgrad+dbn": (dict(res_mode=hip.RES_DBN, stats=True), True), "dgrad+dbn+bias": (dict(res_mode=hip.RES_DBN, stats=True, bias=True), True),
    # the MLP epilogue forms (conv_ref.mlp_epilogue)
    "elu": (dict(act=hip.ACT_ELU), False), "tanh": (dict(act=hip.ACT_TANH), False), "sigmoid": (dict(act=hip.ACT_SIGMOID), False),
    "drop": (dict(drop_p=R.DROP_P, seed=5), False), "bias+elu+drop": (dict(bias=True, act=hip.ACT_ELU, drop_p=R.DROP_P, seed=5), False),
    "dgrad+delu": (dict(res_mode=hip.RES_DELU), True), "dgrad+dtanh": (dict(res_mode=hip.RES_DTANH), True),
    "dgrad+dsigmoid": (dict(res_mode=hip.RES_DSIGMOID), True), "dgrad+delu+drop": (dict(res_mode=hip.RES_DELU, drop_p=R.DROP_P), True),
    "delu": (dict(res_mode=hip.RES_DELU), False), "dtanh": (dict(res_mode=hip.RES_DTANH), False),
    "dsigmoid": (dict(res_mode=hip.RES_DSIGMOID), False),
}
# e4m3 operands (bfloat16 output only: every other descriptor with w_fp8 is refused): e4m3 weights with bfloat16 input (f8) and
# with e4m3 input bytes too (a8), each with the forms a forward layer asks for; and two MLP forms, for the no_copy rule
_F8, _A8 = dict(w_fp8=True, in_scale=R.IN_SCALE), dict(w_fp8=True, in_fp8=True, in_scale=R.IN_SCALE)
for _name, _kw in (("f8", _F8), ("a8", _A8)):
    REQUESTS.update({
        _name: (dict(_kw), False), f"{_name}+bias": (dict(_kw, bias=True), False),
        f"{_name}+bias+relu": (dict(_kw, bias=True, act=hip.ACT_RELU), False), f"{_name}+stats": (dict(_kw, stats=True), False),
        f"{_name}+add": (dict(_kw, res_mode=hip.RES_ADD), False), f"{_name}+drelu": (dict(_kw, res_mode=hip.RES_DRELU), False),
        f"{_name}+shared": (dict(_kw, in_shared=True), False), f"{_name}+addin": (dict(_kw, res_mode=hip.RES_ADD), False), f"{_name}+inbn": (dict(_kw, res_mode=hip.RES_INBN), False),
        f"{_name}+elu": (dict(_kw, act=hip.ACT_ELU), False), f"{_name}+drop": (dict(_kw, drop_p=R.DROP_P, seed=5), False)})
E4M3_REQUESTS = tuple(n for n in REQUESTS if n.split("+")[0] in ("f8", "a8"))


# the single-form requests of the grid -> the flag of conv_ref.CASES that runs the form.  A data gradient is the same kernel under
# another descriptor, so a (code, dtype, form) counts as run whichever of a case's two conv launches carries it.
FORM_OF = {"bias": "bias", "dgrad+bias": "bias", "bias+relu": "relu", "add": "add", "dgrad+add": "add", "dgrad+addin": "addin",
           "drelu": "drelu", "dgrad+drelu": "drelu", "shared": "shared", "stats": "stats",
           **{n: n.split("+")[-1] for n in E4M3_REQUESTS if n.split("+")[-1] in ("f8", "a8", "bias", "relu", "stats", "add", "addin", "drelu", "shared")}}
# the second, coarser rule: the requests that carry an MLP epilogue form -> the forms.  The form's code exists in three copies
# (conv_ref.EPILOGUE_COPY); every (copy, dtype, form) the planner lets a descriptor reach has a case, whichever tile code runs it.
MLP_FORMS_OF = {"elu": ("elu",), "tanh": ("tanh",), "sigmoid": ("sigmoid",), "drop": ("drop",), "bias+elu+drop": ("elu", "drop"),
                "dgrad+delu": ("delu",), "dgrad+dtanh": ("dtanh",), "dgrad+dsigmoid": ("dsigmoid",), "dgrad+delu+drop": ("delu",),
                "delu": ("delu",), "dtanh": ("dtanh",), "dsigmoid": ("dsigmoid",),
                "f8+elu": ("elu",), "f8+drop": ("drop",), "a8+elu": ("elu",), "a8+drop": ("drop",)}


def _grid_plan(lib, E, ipe, cin, cout, side, ks, stride, dtype, name):
    kw, dgrad = REQUESTS[name]
    pad, N = ks // 2, E * ipe
    so = ops.conv_out_size(side, ks, stride, pad)
    if isinstance(kw, str):
        if cout % 32:
            return None
        kw = dict(shuffle2_c=cout // 4, **(dict(res_mode=hip.RES_INBN) if "inbn" in kw else {}))
    if not dgrad:
        d = ops._planning_desc(N, side, side, so, so, cin, cout, R.r64(cout), ipe, ks, stride, pad, dtype, **kw)
    else:
        d = ops._planning_desc(N, so, so, side, side, cout, cin, R.r64(cin), ipe, ks, 1, ks - 1 - pad, dtype, dilate=stride == 2, **kw)
    if name.endswith("+addin"):                                             # accumulated in place: res == out
        d.res = d.out
    return lib.pmoe_conv2d_plan(C.byref(d))


def test_every_plan_code_of_the_grid_has_a_case(monkeypatch):
    """plans only: channels x sides x images per expert x filter x stride x dtype x request x per-launch switch, and a second, narrow
    sweep (SMALL_SIDES x MANY_IPES, 8-channel layers) without switches.  Coverage is per (code, dtype): a code that float32
    reaches needs a float32 case.  The requests with e4m3 operands go through the same rules as every other: no exclusion list."""
    lib = hip.load()
    seen, accepted, accepted_mlp, no_copy = {"conv": set(), "wgrad": set()}, set(), set(), set()
    assert not hasattr(R, "EXCLUDED") and not hasattr(R, "is_excluded"), "there is no exclusion list"

    def conv_sweep(channels, sides, ipes):
        for dtype, cin, cout, side, ipe, ks, stride in itertools.product((torch.bfloat16, torch.float32), channels, channels,
                                                                         sides, ipes, (1, 3), (1, 2)):
            # (e4m3 operands: bfloat16 launches over whole 64-channel chunks; everything else is refused -- asserted below)
            e4m3 = dtype == torch.bfloat16 and cin % 64 == 0
            for name in REQUESTS:
                if name in E4M3_REQUESTS and not e4m3:
                    continue
                code = _grid_plan(lib, 2, ipe, cin, cout, side, ks, stride, dtype, name)
                if code is not None and code >= 0:
                    seen["conv"].add((code, dtype))
                    if name in FORM_OF:
                        accepted.add((code, dtype, FORM_OF[name]))
                    if name in MLP_FORMS_OF:
                        if code not in R.EPILOGUE_COPY:
                            no_copy.add((code, name))
                        accepted_mlp.update((R.EPILOGUE_COPY.get(code), dtype, form) for form in MLP_FORMS_OF[name])
                    assert "inbn" not in name or name not in E4M3_REQUESTS, (code, name)    # (no e4m3 kernel applies a BatchNorm)

    for sw in CONV_SWITCHES:
        with monkeypatch.context() as m:
            if sw:
                m.setenv(*sw)
            conv_sweep(CHANNELS, SIDES, IPES)
    conv_sweep(CHANNELS_8, SMALL_SIDES, MANY_IPES)
    conv_sweep(CHANNELS_8, SIDES[:3], IPES[:2])
    # what the e4m3 requests skip above is refused: float32, and reductions that are no whole 64-channel chunks
    for name in E4M3_REQUESTS:
        assert _grid_plan(lib, 2, 2, 64, 64, 8, 3, 1, torch.float32, name) < 0 and _grid_plan(lib, 2, 2, 32, 64, 8, 3, 1, torch.bfloat16, name) < 0
    for sw in WGRAD_SWITCHES:
        with monkeypatch.context() as m:
            if sw:
                m.setenv(*sw)
            for dtype, cin, cout, side, ipe, ks, stride in itertools.product((torch.bfloat16, torch.float32), CHANNELS, CHANNELS,
                                                                             SIDES, IPES, (1, 3), (1, 2)):
                ckw = 64 if dtype == torch.bfloat16 else 32
                so = ops.conv_out_size(side, ks, stride, ks // 2)
                for per_image, bn in ((False, False), (True, False), (True, True)):
                    d = ops._wgrad_desc(2 * ipe, side, side, so, so, cin, cout, (cin + ckw - 1) // ckw * ckw, (cout + ckw - 1) // ckw * ckw,
                                        ipe, ks, stride, ks // 2, hip._TORCH_DT[dtype], per_image=per_image, bn_z_ld=0 if bn else None)
                    code = lib.pmoe_conv2d_wgrad_plan(C.byref(d))
                    if code >= 0:
                        seen["wgrad"].add((code, dtype))
    covered = {"conv": {(c, case.dtype) for case in R.CASES for c in case.codes[:2] if c is not None},
               "wgrad": {(case.codes[2], case.dtype) for case in R.CASES if case.codes[2] is not None}}
    for k in seen:
        missing = sorted((c, str(d)) for c, d in seen[k] - covered[k])
        assert not missing, f"{k} (plan code, dtype) without a case: {missing}"
        print(k, "codes seen:", sorted((c, str(d)) for c, d in seen[k]))
    # the table names nothing the grid does not know (a stale code would be a case that runs on something else)
    assert covered["conv"] <= seen["conv"] and covered["wgrad"] <= seen["wgrad"], sorted(
        (c, str(d)) for c, d in (covered["conv"] - seen["conv"]) | (covered["wgrad"] - seen["wgrad"]))
    conv_codes = {c for c, _ in covered["conv"]}
    assert conv_codes <= set(R.ROUNDING), sorted(conv_codes - set(R.ROUNDING))
    assert {742, 4742, 8742, 8507, 8622, 8641, 8642, 8722, 8741, 10007} <= conv_codes
    # every form on every code (and dtype) whose planner accepts it, and channel windows on every code
    ran, windowed = set(), set()
    for case in R.CASES:
        fl = R.flags(case)
        for i, k in enumerate("fd"):
            if fl[k] is not None:
                ran |= {(case.codes[i], case.dtype, form) for form in fl[k]}
                if "win" in fl[k]:
                    windowed.add(case.codes[i])
    missing = sorted((c, str(d), f) for c, d, f in accepted - ran)
    assert not missing, f"(code, dtype, form) accepted by the planner and run by no case: {missing}"
    unwindowed = sorted(conv_codes - windowed)
    assert not unwindowed, f"plan codes no case runs on channel windows: {unwindowed}"
    # the MLP epilogue forms: only the kernels that carry a copy of that epilogue ever answer a descriptor that asks for one, and
    # every (copy, dtype, form) the grid reaches is run by a case
    assert not no_copy, f"MLP forms planned onto codes outside conv_ref.EPILOGUE_COPY: {sorted(no_copy)}"
    ran_mlp = set()
    for case in R.CASES:
        fl = R.flags(case)
        for i, k in enumerate("fd"):
            for form in (fl[k] or ()):
                form = "drop" if form in R.DROP_FLAGS and k == "f" else form
                if form in R.ACT_FLAGS or form in R.DMODE_FLAGS or form == "drop":
                    assert case.codes[i] in R.EPILOGUE_COPY, (case, k)
                    ran_mlp.add((R.EPILOGUE_COPY[case.codes[i]], case.dtype, form))
    print("MLP forms reached on the grid:", sorted((c, str(d), f) for c, d, f in accepted_mlp))
    assert {c for c, _, _ in accepted_mlp} == set(R.EPILOGUE_COPY.values()), "a copy of the epilogue that no MLP form reaches"
    missing = sorted((c, str(d), f) for c, d, f in accepted_mlp - ran_mlp)
    assert not missing, f"(epilogue copy, dtype, form) accepted by the planner and run by no case: {missing}"


# ---------------------------------------------------------------------------------------------------------------------------------
# generator properties

def _representable(t, dtype):
    return torch.equal(t.to(dtype).to(F64)[~torch.isnan(t)], t[~torch.isnan(t)])


def case_kinds(cases, kinds=R.KINDS + (R.DYADIC, R.SELECT)):
    """(case, kind) for every kind the case runs on, with the ids the two stacked parametrisations gave before the dyadic kind"""
    return dict(argnames="case,kind", argvalues=[(c, k) for k in kinds for c in cases if k in R.kinds_of(c)],
                ids=[f"{R.case_id(c)}-{k}" for k in kinds for c in cases if k in R.kinds_of(c)])


@pytest.mark.parametrize(**case_kinds(R.CASES, R.KINDS))
def test_generator_properties(case, kind):
    ls = R.launches(case, kind)
    dtype = case.dtype
    for k in ("f", "d"):
        if k not in ls:
            continue
        L = ls[k]
        kw = L["kw"]
        for name in ("inp", "w", "out_init", "res"):
            assert L[name] is None or _representable(L[name], dtype), (k, name)
        for name in ("bias", "bn_coef"):
            assert L[name] is None or _representable(L[name], F32), (k, name)
        bound = R.abs_bound(L)
        assert bound < 2 ** 24, (k, bound)
        if L.get("f8"):
            check_e4m3_operands(L, fixed_point=True)
        ref = R.conv_reference(L)
        # float32 in two orders == float64, bit for bit (INBN: the operand is the reference's own)
        xw = L["inp"][..., kw["in_coff"]:kw["in_coff"] + kw["cin"]]
        if kw.get("res_mode") == R.RES_INBN:
            c = L["bn_coef"]
            xw = bn_ref.bn_apply(xw, None, c[2], c[3], c[0], c.shape[1], True, dtype)["y"]
        ho, wo = ref["acc"].shape[1:3]
        geo = dict(ipe=kw["ipe"], in_shared=kw.get("in_shared", False), stride=kw["stride"], pad=kw["pad"], ho=ho, wo=wo,
                   dilate=kw.get("dilate", False))
        for taps in (False, True):
            a32 = R.conv_acc(xw, L["w"], dtype=F32, taps=taps, **geo)
            assert torch.equal(a32.to(F64), ref["acc"]), (k, "float32 accumulation differs from float64", taps)
        stored, pre = ref["stored"], ref["pre"]
        if kind == "unit":
            assert pre.abs().max() < 256 and torch.equal(stored, pre), (k, pre.abs().max().item())
            if kw["stats"]:
                assert (ref["sums_abs"] < 2 ** 24).all(), k                   # (integer terms: the unit kind's x-hat is one too)
        elif dtype == BF16:
            # (of the elements the launch computes and keeps: the in-place 1x1 form computes a quarter of the pixels, a mask
            #  clears its share)
            nz = (ref["acc"] != 0) & (pre != 0)
            inexact = (stored != pre)
            tie = inexact & (bf16_boundary_distance(pre.abs()) == 0)
            fi, ft = inexact.sum().item() / nz.sum().item(), tie.sum().item() / nz.sum().item()
            print(f"{k}: {100 * fi:.1f} % of the non-zero outputs round, {100 * ft:.1f} % on exact ties; max sum|x||w| {bound:.0f}")
            assert fi >= 0.05 and ft >= 0.05, (k, fi, ft)
        mode, fl = kw.get("res_mode"), R.flags(case)[k]
        if kw.get("act") == R.ACT_RELU:
            edge = ref["acc"][0, min(2, ho - 1) // kw["stride"], min(2, wo - 1) // kw["stride"]] + L["bias"][0]
            if mode == R.RES_ADD:                                               # (a separate residual is zero on the planted pixel)
                res = L["out_init"] if L["res_is_out"] else L["res"]
                edge = edge + res[0, min(2, ho - 1) // kw["stride"], min(2, wo - 1) // kw["stride"], kw["res_coff"]:kw["res_coff"] + kw["cout"]]
            assert L["res_is_out"] or all((edge == v).any() for v in (-1.0, 0.0, 1.0)), k
            assert (pre == 0).any() and (ref["acc"] > 0).any() and (ref["acc"] < 0).any()
        if mode in (R.RES_DBN, R.RES_INBN):
            c = L["bn_coef"]
            z = xw if mode == R.RES_INBN else L["res"][..., kw["res_coff"]:kw["res_coff"] + kw["cout"]]
            zin = L["inp"][..., kw["in_coff"]:kw["in_coff"] + kw["cin"]] if mode == R.RES_INBN else z
            p = (zin - R._per_image(c[0], kw["bn_ipe"])) * R._per_image(c[2], kw["bn_ipe"]) + R._per_image(c[3], kw["bn_ipe"])
            step = (R._per_image(c[2], kw["bn_ipe"]) * (1.0 if kind == "unit" else 0.25)).abs()
            assert (p == 0).any() and (p == step).any() and (p == -step).any(), k
        if mode == R.RES_DRELU:
            r = L["res"][..., kw["res_coff"]:kw["res_coff"] + kw["cout"]]
            assert all((r == v).any() for v in (-1.0, 0.0, 1.0)), k
    if "w" in ls:
        L = ls["w"]
        assert _representable(L["x"], dtype) and _representable(L["dy"], dtype)
        ref = R.wgrad_reference(L)
        if L["bn"] is not None:
            z, coef, c1, c2 = L["bn"]
            assert _representable(z, dtype) and all(_representable(t, F32) for t in (coef, c1, c2))
            raw = bn_ref.bn_bwd_apply(L["dy"], None, z, coef[0], coef[1], coef[2], coef[3], c1, c2, case.E, False, F64)["dx"]
            assert ((ref["dz"] != raw).float().mean() > 0.05), "the fused BatchNorm backward's bfloat16 rounding never rounds"
        kw = L["kw"]
        mags = R.wgrad(L["x"].abs(), ref["dz"].abs() if L["bn"] is not None else L["dy"].abs(),
                       **{**kw, "dy_coff": 0 if L["bn"] is not None else kw["dy_coff"]})["dw_ws"]
        unit = 2048 if L["bn"] is not None else 1                           # (dz: multiples of 2^-11)
        assert mags.max() * unit < 2 ** 24, mags.max().item()
        assert torch.equal(R.wgrad_reference(L, evaluate=F32)["dw_ws"].to(F64), ref["dw_ws"])


# ---------------------------------------------------------------------------------------------------------------------------------
# e4m3 operands: the fixed-point property of the lattice and unit kinds, the operands the GPU test feeds, the select kind

F8_CASES = [c for c in R.CASES if R.SELECT in R.kinds_of(c)]


def _same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


def check_e4m3_operands(L, fixed_point):
    """what conv_ref.e4m3_operands hands the kernel decodes to what the reference convolves: bytes x scales == the quantised
    operands (fixed_point: == the launch's own input and weights, the quantisers change nothing); pad rows zero, out_scale NaN
    past cout, 0x7f outside the input window; in_scale a power of two under which nothing saturates unless the kind means it to"""
    kw, s_in = L["kw"], L["in_scale"]
    cin, cout, c0 = kw["cin"], kw["cout"], kw["in_coff"]
    coutp = R.r64(cout)
    qi, qw = R.operands(L)
    if fixed_point:
        assert _same_with_nan(qi, L["inp"]) and torch.equal(qw, L["w"]), "the generator is no fixed point of the e4m3 quantisers"
        assert L["inp"][..., c0:c0 + cin].abs().max() * s_in <= 448
    assert torch.equal(qw, R.qdq_weight(qw)) and _same_with_nan(qi, R.qdq_act(qi, s_in))
    assert s_in > 0 and torch.frexp(torch.tensor(s_in))[0] == 0.5
    wb, osc, xb = R.e4m3_operands(L, coutp)
    E, ks = L["w"].shape[0], kw["ks"]
    assert wb.shape == (E, coutp, ks * ks, cin) and wb[:, cout:].abs().sum() == 0
    assert torch.isnan(osc[:, cout:]).all() and not torch.isnan(osc[:, :cout]).any()
    assert torch.equal(torch.frexp(osc[:, :cout])[0], torch.full((E, cout), 0.5)), "out_scale: powers of two"
    deq = wb[:, :cout].view(torch.float8_e4m3fn).to(F64) * (osc[:, :cout].to(F64) * s_in)[:, :, None, None]
    assert torch.equal(deq.permute(0, 1, 3, 2).reshape(qw.shape), qw)
    if L["a8"]:
        outside = torch.ones(xb.shape[-1], dtype=torch.bool)
        outside[c0:c0 + cin] = False
        assert (xb[..., outside] == 0x7f).all() and xb.shape == L["inp"].shape
        assert torch.equal(xb[..., c0:c0 + cin].view(torch.float8_e4m3fn).to(F64) / s_in, qi[..., c0:c0 + cin])
    else:
        assert xb is None


def test_one_e4m3_case_runs_under_another_in_scale():
    scales = {R.launches(c, "unit")["f"]["in_scale"] for c in F8_CASES}
    assert R.IN_SCALE in scales and len(scales) > 1


@pytest.mark.parametrize(**case_kinds(F8_CASES, (R.SELECT,)))
def test_select_generator_properties(case, kind):
    """what tests/test_conv_gpu.py assumes of the select kind: one non-zero +-2^j per filter row, e4m3-exact after its row scale; the
    planted input classes all inside the channel window; the accumulator one product per element -- +-2^j times the converted
    input at the shifted pixel, 0 in the padding -- exact in bfloat16, and every float32 sum of the tail behind it exact"""
    L = R.launches(case, kind)["f"]
    kw, s_in = L["kw"], L["in_scale"]
    cin, cout, c0, ks, stride, pad = kw["cin"], kw["cout"], kw["in_coff"], kw["ks"], kw["stride"], kw["pad"]
    for name in ("inp", "w", "out_init", "res"):
        assert L[name] is None or _representable(L[name], BF16), name
    assert L["bias"] is None or _representable(L["bias"], F32)
    check_e4m3_operands(L, fixed_point=False)
    w = L["w"]
    E = w.shape[0]
    flat = w.reshape(E, cout, -1)
    assert ((flat != 0).sum(2) == 1).all(), "one non-zero per row"
    val, at = flat.gather(2, flat.abs().argmax(2, keepdim=True))[..., 0], flat.abs().argmax(2)
    assert torch.equal(torch.frexp(val.abs())[0], torch.full_like(val, 0.5)) and (val > 0).any() and (val < 0).any()
    assert torch.equal(R.qdq_weight(w), w), "the scaled weight is e4m3-exact"
    assert len(torch.unique(at % (ks * ks))) == ks * ks, "every tap is selected by some channel"
    # the planted classes, inside the window; NaN outside it
    outside = torch.ones(L["inp"].shape[-1], dtype=torch.bool)
    outside[c0:c0 + cin] = False
    assert torch.isnan(L["inp"][..., outside]).all()
    xw = L["inp"][..., c0:c0 + cin]
    s = xw * s_in
    present = lambda vals: bool(torch.isin(vals, s).all())
    if L["a8"]:
        codes = torch.unique(R.e4m3_operands(L, R.r64(cout))[2][..., c0:c0 + cin])
        assert codes.numel() == 254 and 0x7f not in codes and 0xff not in codes, "all 254 non-NaN byte codes"
    else:
        v = R.e4m3_values()
        ties = (v[:-1] + v[1:]) / 2
        for sign in (1, -1):
            assert present(sign * v) and present(sign * ties), "every e4m3 value and every tie, both signs"
            assert present(sign * R.bf16_neighbour(ties, 1)) and present(sign * R.bf16_neighbour(ties, -1)), "the ties' bf16 neighbours"
            assert ((sign * s > 0) & (s.abs() < 2.0 ** -10)).any(), "below half the smallest subnormal"
            assert (sign * s > 448).any() and (sign * s).max() >= 1.5e5, "beyond 448 up to 1e4 x 16"
        assert (v[1:8] == torch.arange(1, 8) * 2.0 ** -9).all() and ties[0] == 2.0 ** -10, "seven subnormals; the first tie"
        q = R.qdq_act(xw, s_in) * s_in
        assert q.abs().max() == 448 and ((q == 0) & (xw != 0)).any() and present(torch.tensor([464.0], dtype=F64))
    assert ((xw == 0) & torch.signbit(xw)).any() and ((xw == 0) & ~torch.signbit(xw)).any(), "both zeros"
    # one product per element
    ref = R.conv_reference(L)
    acc = ref["acc"]
    n, ho, wo = acc.shape[:3]
    xq = R.qdq_act(xw, s_in)
    span_y, span_x = (ho - 1) * stride + ks, (wo - 1) * stride + ks
    xp = F.pad(xq, (0, 0, pad, max(span_x - xq.shape[2] - pad, 0), pad, max(span_y - xq.shape[1] - pad, 0)))
    want = torch.empty_like(acc)
    ipe = kw["ipe"]
    for e in range(E):
        xe = xp[:ipe] if kw["in_shared"] else xp[e * ipe:(e + 1) * ipe]
        for co in range(cout):
            ci, ky, kx = int(at[e, co]) // (ks * ks), int(at[e, co]) % (ks * ks) // ks, int(at[e, co]) % ks
            want[e * ipe:(e + 1) * ipe, :, :, co] = val[e, co] * xe[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, ci]
    assert torch.equal(acc, want), "the accumulator is not the selected, converted input"
    assert torch.equal(R.round_to(acc, BF16), acc) and R.abs_bound(L) < 2 ** 24
    assert (acc != 0).float().mean() > 0.5 and acc.abs().max() <= 448 / s_in * 4
    # the float32 tail: out_scale (a power of two), bias, side input -- every sum exact, so the one rounding is the bfloat16 one
    v = acc
    if L["bias"] is not None:
        v = v + L["bias"].repeat_interleave(ipe, 0)[:, None, None, :]
        assert torch.equal(R._f32(v), v), "acc + bias rounds in float32"
    if kw.get("res_mode") == R.RES_ADD:
        res = L["out_init"] if L["res_is_out"] else L["res"]
        v = v + res[..., kw["res_coff"]:kw["res_coff"] + cout]
        assert torch.equal(R._f32(v), v), "acc + bias + res rounds in float32"
    if kw["stats"]:
        assert (ref["sums_abs"] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference against torch and its autograd (continuous float64 data, one small shape per form)

def relerr(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 7, 9, 3, 1), (1, 2, 4, 6, 9, 7, 3, 2), (2, 2, 6, 4, 8, 8, 3, 2), (2, 1, 5, 3, 7, 6, 1, 2),
                                   (1, 3, 4, 8, 5, 5, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_reference_matches_autograd(shape):
    """forward with bias / residual / ReLU / statistics, the data gradient as the launch forms it (flipped transposed filter,
    zero-dilated source at stride 2, accumulated in place) and the weight gradient with its workspace layout"""
    E, ipe, cin, cout, H, W, ks, stride = shape
    g = torch.Generator().manual_seed(sum(shape))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    N, pad = E * ipe, ks // 2
    Ho, Wo = R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad)
    x, w, b, res, dy, prev = rn(N, H, W, cin), rn(E, cout, cin, ks, ks), rn(E, cout), rn(N, Ho, Wo, cout), rn(N, Ho, Wo, cout), rn(N, H, W, cin)
    xr, wr, br = nchw(x).clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lin = torch.cat([F.conv2d(xr[e * ipe:(e + 1) * ipe], wr[e], br[e], stride=stride, padding=pad) for e in range(E)])
    y = F.relu(lin + nchw(res))
    y.backward(nchw(dy))
    buf, coff = R._window(x, True)
    out_init = torch.full((N, Ho, Wo, cout + 8), R.SENTINEL, dtype=F64)
    f = R.conv2d(buf, w, out_init, cin=cin, cout=cout, ipe=ipe, ks=ks, stride=stride, pad=pad, dtype=F64, in_coff=coff, out_coff=8,
                 bias=b, res=res, res_mode=R.RES_ADD, act=R.ACT_RELU, stats=True)
    assert relerr(nchw(f["stored"]), y.detach()) < 1e-12 and relerr(nchw(f["acc"]), (lin - br.repeat_interleave(ipe, 0)[:, :, None, None]).detach()) < 1e-12
    assert (f["out"][..., :8] == R.SENTINEL).all() and torch.equal(f["out"][..., 8:], f["stored"])
    ye = nhwc(y.detach()).reshape(E, -1, cout)
    assert relerr(f["sums"][:, 0], ye.sum(1)) < 1e-12 and relerr(f["sums"][:, 1], (ye * ye).sum(1)) < 1e-12
    # data gradient: g = dy masked by the ReLU (PMOE_RES_DRELU on the saved output is that mask applied to a convolution)
    gm = dy * (f["stored"] > 0)
    wd = w.flip(3, 4).transpose(1, 2).contiguous()
    dgr = R.conv2d(gm, wd, prev, cin=cout, cout=cin, ipe=ipe, ks=ks, stride=1, pad=ks - 1 - pad, dtype=F64, dilate=stride == 2,
                   res=prev, res_mode=R.RES_ADD)
    assert relerr(nchw(dgr["out"]), xr.grad + nchw(prev)) < 1e-12
    fwd, dgrd = R.pack_weights(w, cout + 3, cin + 2, F64, cin + 1, cout + 5)
    assert torch.equal(dgrd[:, :cin, :, :cout], wd.reshape(E, cin, cout, ks * ks).permute(0, 1, 3, 2))
    assert torch.equal(fwd[:, :cout, :, :cin], w.reshape(E, cout, cin, ks * ks).permute(0, 1, 3, 2)) and fwd[:, cout:].abs().sum() == 0
    # weight gradient
    wg = R.wgrad(x, gm, cin=cin, cout=cout, cinp=cin + 3, coutp=cout + 2, ipe=ipe, ks=ks, stride=stride, pad=pad, dtype=F64)
    assert relerr(wg["grads"], wr.grad) < 1e-12
    assert wg["dw_ws"].shape == (E, ks * ks, cout + 2, cin + 3) and wg["dw_ws"][:, :, cout:].abs().sum() == 0
    pi = R.wgrad(x, gm, cin=cin, cout=cout, cinp=cin + 3, coutp=cout + 2, ipe=ipe, ks=ks, stride=stride, pad=pad, dtype=F64, per_image=True)
    assert relerr(pi["dw_ws"].reshape(E, ipe, ks * ks, cout + 2, cin + 3).sum(1), wg["dw_ws"]) < 1e-12
    if stride == 1:
        # a shared input: every expert reads the same ipe images
        xs = x[:ipe]
        sh = R.conv2d(xs, w, out_init[..., :cout], cin=cin, cout=cout, ipe=ipe, ks=ks, stride=1, pad=pad, dtype=F64, in_shared=True)
        want = torch.cat([F.conv2d(nchw(xs), w[e], padding=pad) for e in range(E)])
        assert relerr(nchw(sh["stored"]), want) < 1e-12
        ws = R.wgrad(xs, gm, cin=cin, cout=cout, cinp=cin, coutp=cout, ipe=ipe, ks=ks, stride=1, pad=pad, dtype=F64, x_shared=True)
        xr2, w2 = nchw(xs).clone(), w.clone().requires_grad_(True)
        torch.cat([F.conv2d(xr2, w2[e], padding=pad) for e in range(E)]).backward(nchw(gm))
        assert relerr(ws["grads"], w2.grad) < 1e-12


def test_reference_shuffle_matches_conv_transpose():
    E, ipe, cin, c_up, H, W = 2, 2, 6, 8, 4, 8
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, wt, b = rn(E * ipe, H, W, cin), rn(E, cin, c_up, 2, 2), rn(E, c_up)
    # the 1x1 layer of include/pmoe_hip.h: row (2 dy + dx) * c_up + c of its filter
    w = wt.permute(0, 3, 4, 2, 1).reshape(E, 4 * c_up, cin, 1, 1)
    out_init = torch.full((E * ipe, 2 * H, 2 * W, 2 * c_up), R.SENTINEL, dtype=F64)
    r = R.conv2d(x, w, out_init, cin=cin, cout=4 * c_up, ipe=ipe, ks=1, stride=1, pad=0, dtype=F64, out_coff=c_up, shuffle_c=c_up,
                 bias=b.repeat(1, 4))
    want = torch.cat([F.conv_transpose2d(nchw(x[e * ipe:(e + 1) * ipe]), wt[e], b[e], stride=2) for e in range(E)])
    assert relerr(nchw(r["out"][..., c_up:]), want) < 1e-12 and (r["out"][..., :c_up] == R.SENTINEL).all()


def test_reference_fused_batchnorm_forms_match_batch_norm_and_autograd():
    """PMOE_RES_INBN forward, PMOE_RES_DBN data gradient with its two reductions, and the bn_fused weight gradient against
    conv -> batch_norm -> relu -> conv in float64 autograd"""
    E, ipe, C, H, W, eps = 2, 3, 5, 6, 7, 1e-5
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    N = E * ipe
    x, w1, w2, dy = rn(N, H, W, C), rn(E, C, C, 3, 3), rn(E, C, C, 3, 3), rn(N, H, W, C)
    gamma, beta = 1 + 0.1 * rn(E, C), 0.1 * rn(E, C)
    xr, w1r, gr, br = nchw(x).clone().requires_grad_(True), w1.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    zs, outs = [], []
    for e in range(E):
        z = F.conv2d(xr[e * ipe:(e + 1) * ipe], w1r[e], padding=1)
        zs.append(z)
        outs.append(F.conv2d(F.relu(F.batch_norm(z, None, None, gr[e], br[e], True, 0.1, eps)), w2[e], padding=1))
    torch.cat(outs).backward(nchw(dy))
    z = nhwc(torch.cat(zs).detach()).contiguous()
    ze = z.reshape(E, -1, C)
    mean, var = ze.mean(1), ze.var(1, unbiased=False)
    invstd = 1 / torch.sqrt(var + eps)
    coef = torch.stack([mean, invstd, gamma * invstd, beta])
    blank = torch.zeros(N, H, W, C, dtype=F64)
    f = R.conv2d(z, w2, blank, cin=C, cout=C, ipe=ipe, ks=3, stride=1, pad=1, dtype=F64, res_mode=R.RES_INBN, bn_coef=coef, bn_ipe=ipe)
    assert relerr(nchw(f["stored"]), torch.cat(outs).detach()) < 1e-11
    wd = w2.flip(3, 4).transpose(1, 2).contiguous()
    d = R.conv2d(dy, wd, blank, cin=C, cout=C, ipe=ipe, ks=3, stride=1, pad=1, dtype=F64, res=z, res_mode=R.RES_DBN, bn_coef=coef,
                 bn_ipe=ipe, stats=True)
    assert relerr(d["sums"][:, 0], br.grad) < 1e-11 and relerr(d["sums"][:, 1], gr.grad) < 1e-11
    fin = bn_ref.bn_bwd_finalize(d["sums"][:, None], ipe * H * W)
    wg = R.wgrad(x, d["stored"], cin=C, cout=C, cinp=C, coutp=C, ipe=ipe, ks=3, stride=1, pad=1, dtype=F64,
                 bn=(z, coef, fin["c1"], fin["c2"]))
    assert relerr(wg["grads"], w1r.grad) < 1e-10
    dz = bn_ref.bn_bwd_apply(d["stored"], None, z, mean, invstd, coef[2], beta, fin["c1"], fin["c2"], E, False, F64)["dx"]
    wd1 = w1.flip(3, 4).transpose(1, 2).contiguous()
    dx = R.conv2d(dz, wd1, blank, cin=C, cout=C, ipe=ipe, ks=3, stride=1, pad=1, dtype=F64)
    assert relerr(nchw(dx["stored"]), xr.grad) < 1e-10


def test_reference_scaled_and_gated_packs():
    E, ipe, cout, cin, ks = 2, 3, 4, 5, 3
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    w, sc, sh, mu, gate, x = rn(E, cout, cin, ks, ks), rn(E, cout), rn(E, cout), rn(E, cout), rn(E * ipe, cin + 2), rn(E * ipe, 6, 6, cin)
    fwd, bias = R.pack_weights_scaled(w, sc, sh, mu, cout, cin, F64)
    blank = torch.zeros(E * ipe, 6, 6, cout, dtype=F64)
    unpack = lambda p: p.permute(0, 1, 3, 2).reshape(p.shape[0], cout, cin, ks, ks)
    y = R.conv2d(x, unpack(fwd), blank, cin=cin, cout=cout, ipe=ipe, ks=ks, stride=1, pad=1, dtype=F64, bias=bias)["stored"]
    plain = R.conv2d(x, w, blank, cin=cin, cout=cout, ipe=ipe, ks=ks, stride=1, pad=1, dtype=F64)["stored"]
    bc = lambda t: t.repeat_interleave(ipe, 0)[:, None, None, :]
    assert relerr(y, (plain - bc(mu)) * bc(sc) + bc(sh)) < 1e-12                 # eval-mode BatchNorm folded into the filter
    gf, gd = R.pack_weights_gated(w, gate, ipe, cout, cin, F64, cin, cout)
    yg = R.conv2d(x, unpack(gf), blank, cin=cin, cout=cout, ipe=1, ks=ks, stride=1, pad=1, dtype=F64)["stored"]
    want = R.conv2d(x * gate[:, None, None, :cin], w, blank, cin=cin, cout=cout, ipe=ipe, ks=ks, stride=1, pad=1, dtype=F64)["stored"]
    assert relerr(yg, want) < 1e-12
    assert torch.equal(gd, R.pack_weights(unpack(gf), cout, cin, F64, cin, cout)[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the MLP epilogue forms: the dyadic generator, the reference against autograd, the skinny GEMM's row limit, the mutants

DYADIC_CASES = [c for c in R.CASES if R.kinds_of(c) == (R.DYADIC,)]
AMBIGUOUS_CAP = 0.02


def test_edge_seed_makes_one_hash_equal_p():
    p = torch.tensor(R.DROP_P, dtype=F32).to(F64)
    u = H.hash_uniform(R.SEED_OF["dropE"], R.EDGE_INDEX + 2)
    assert u[R.EDGE_INDEX] == p and (u != p).sum() == R.EDGE_INDEX + 1
    assert R.SEED_OF["dropL"] > 2 ** 32 > R.SEED_OF["drop"] and R.SEED_OF["dropE"] > 2 ** 32


@pytest.mark.parametrize(**case_kinds(DYADIC_CASES, (R.DYADIC,)))
def test_dyadic_generator_properties(case, kind):
    """what tests/test_conv_gpu.py assumes of the dyadic kind: representable, sums exact in any order, pre-activations spread over
    the unsaturated range with exact zeros, saved outputs on both sides with dropped zeros, few outputs whose stored value the
    allowance leaves open"""
    ls = R.launches(case, kind)
    dtype = case.dtype
    for k in ("f", "d"):
        if k not in ls:
            continue
        L = ls[k]
        kw = L["kw"]
        for name in ("inp", "w", "out_init", "res"):
            assert L[name] is None or _representable(L[name], dtype), (k, name)
        assert L["bias"] is None or _representable(L["bias"], F32)
        bound = R.abs_bound(L)
        assert bound * 64 < 2 ** 24, (k, bound)                               # (every term a multiple of 1/64)
        ref = R.conv_reference(L)
        xw = L["inp"][..., kw["in_coff"]:kw["in_coff"] + kw["cin"]]
        ho, wo = ref["acc"].shape[1:3]
        geo = dict(ipe=kw["ipe"], in_shared=kw.get("in_shared", False), stride=kw["stride"], pad=kw["pad"], ho=ho, wo=wo,
                   dilate=kw.get("dilate", False))
        for taps in (False, True):
            assert torch.equal(R.conv_acc(xw, L["w"], dtype=F32, taps=taps, **geo).to(F64), ref["acc"]), (k, taps)
        pre, allow = ref["pre"], ref["allow"]
        assert (allow >= 0).all() and torch.equal(pre[allow == 0], R._f32(pre[allow == 0])), "an exact element is a float32 value"
        lo, hi = R.stored_interval(ref, dtype)
        nz = ref["stored"] != 0
        open_ = ((lo != hi) & nz).sum().item() / max(nz.sum().item(), 1)
        print(f"{k}: {nz.sum().item()} non-zero outputs, {100 * (allow[nz] == 0).float().mean().item():.1f} % exact, "
              f"{100 * open_:.3f} % with two possible stored values; max sum|x||w| {bound:.1f}")
        if dtype == BF16:
            assert open_ <= AMBIGUOUS_CAP, (k, open_)
        drop, act, mode = kw.get("drop_p", 0.0) > 0, kw.get("act", R.ACT_NONE), kw.get("res_mode", R.RES_NONE)
        if k == "f":
            v = ref["acc"] if L["bias"] is None else ref["acc"] + L["bias"].repeat_interleave(kw["ipe"], 0)[:, None, None, :]
            if act >= R.ACT_ELU:
                share = [((v > a) & (v <= b) if a < -1 else (v >= a) & (v < b) if a >= 1 else (v > a) & (v < b)).float().mean().item()
                         for a, b in ((-8, -1), (-1, 0), (0, 1), (1, 8))]
                print(f"f: pre-activations in (-8, -1], (-1, 0), (0, 1), [1, 8): {[round(s, 3) for s in share]}, "
                      f"{torch.unique(v).numel()} distinct")
                assert min(share) >= 0.10, share
            assert (v == 0).any() and (v > 0).any() and (v < 0).any()
            if drop:
                assert 0.6 < ref["keep"].float().mean().item() < 0.8 and (ref["undropped"][~ref["keep"]] != 0).any()
            if kw.get("seed") == R.SEED_OF["dropE"]:
                e = R.EDGE_INDEX
                assert ref["keep"].flatten()[e] and ref["stored"].flatten()[e] != 0, "the element whose hash equals p is kept and shows"
        else:
            r = L["res"][..., kw["res_coff"]:kw["res_coff"] + kw["cout"]]
            u = r / H.keep_scale(kw.get("drop_p", 0.0), F64)
            mid = 0.5 if mode == R.RES_DSIGMOID else 0.0
            assert (u > mid).any() and ((u < mid) & (r != 0)).any() or mode == R.RES_DRELU and (r > 0).any(), k
            assert (r == 0).any() or (mode == R.RES_DSIGMOID and not drop), k           # (a sigmoid is zero only where dropped)
            if drop:
                assert ((r == 0) & (L["saved_z"] != 0)).any() and ((r != 0) & (ref["stored"] != 0)).any(), k


@pytest.mark.parametrize("p", [0.0, R.DROP_P])
@pytest.mark.parametrize("act", ["relu", "elu", "tanh", "sigmoid"])
def test_reference_mlp_forms_match_autograd(act, p):
    """act(linear) * mask * keep_scale and its data gradient from the saved output, against float64 autograd under the
    reference's own mask (continuous data: the float32 roundings of the exact paths stay below 1e-6)"""
    E, ipe, cin, cout = 2, 9, 6, 8
    g = torch.Generator().manual_seed(17)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    N = E * ipe
    x, w, b, dy = rn(N, 1, 1, cin), rn(E, cout, cin, 1, 1), rn(E, cout), rn(N, 1, 1, cout)
    geo = dict(ipe=ipe, ks=1, stride=1, pad=0, dtype=F64, drop_p=p, seed=5)
    blank = torch.zeros(N, 1, 1, cout, dtype=F64)
    f = R.conv2d(x, w, blank, cin=cin, cout=cout, bias=b, act=hip.ACT_BY_NAME[act], **geo)
    xr = x.clone().requires_grad_(True)
    z = torch.cat([F.linear(xr[e * ipe:(e + 1) * ipe], w[e, :, :, 0, 0], b[e]) for e in range(E)])
    y = {"relu": F.relu, "elu": F.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](z) * f["keep"] * H.keep_scale(p, F64)
    y.backward(dy)
    assert relerr(f["stored"], y.detach()) < 1e-6
    assert p == 0 or 0.5 < f["keep"].float().mean() < 0.9
    # the launch the engine runs: the gradient w.r.t. z of layer l is the data gradient of layer l + 1 times act'(saved output)
    up = rn(N, 1, 1, cin)
    w2 = rn(E, cout, cin, 1, 1)
    h = R.conv2d(up, w2, blank, cin=cin, cout=cout, res=f["stored"], res_mode=hip.RES_OF_ACT[hip.ACT_BY_NAME[act]], **geo)
    lin = R.conv2d(up, w2, blank, cin=cin, cout=cout, ipe=ipe, ks=1, stride=1, pad=0, dtype=F64)["stored"]
    zr = z.detach().clone().requires_grad_(True)
    ({"relu": F.relu, "elu": F.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](zr) * f["keep"] * H.keep_scale(p, F64)).backward(lin)
    assert relerr(h["stored"], zr.grad) < 1e-6 and (h["allow"] >= 0).all()


def test_skinny_row_limit():
    """3200 output rows per expert plan to the skinny GEMM, 3280 do not (conv_ref.CASES runs the first)"""
    plan = lambda W: ops.conv2d_plan(2, 40, W, 40, W, 16, 16, 64, 2, 1, 1, 0, torch.bfloat16)
    assert plan(40) == 3000
    assert plan(41) >= 0 and plan(41) != 3000


def test_every_mutant_is_told_apart():
    """each deliberately wrong variant of conv_ref.MUTANTS leaves the reference's interval of stored values on at least one launch
    of the skinny-GEMM and MLP-form cases: the inputs can tell it from the kernel's contract.  And the select kind tells the two
    mutants of the main loop apart on the cases with e4m3 operands"""
    cases = [c for c in R.CASES if 3000 in c.codes[:2] or c in DYADIC_CASES]
    caught = {}
    for case in cases:
        for kind in R.kinds_of(case):
            ls = R.launches(case, kind)
            for k in ("f", "d"):
                if k not in ls:
                    continue
                ref = R.conv_reference(ls[k])
                lo, hi = R.stored_interval(ref, case.dtype)
                for mut in R.MUTANTS:
                    if mut in caught:
                        continue
                    got = R.conv_reference(ls[k], mut=mut)["stored"]
                    n = int(((got < lo) | (got > hi)).sum())
                    if n:
                        caught[mut] = f"{R.case_id(case)}-{kind} {k}: {n} elements"
        if len(caught) == len(R.MUTANTS):
            break
    print("\n".join(f"{m}: {w}" for m, w in caught.items()))
    assert not set(R.MUTANTS) - set(caught), f"mutants no case tells apart: {sorted(set(R.MUTANTS) - set(caught))}"
    # the select kind of the cases with e4m3 operands, where equality is the GPU test's criterion: a dropped k-slice and a tap that
    # reads the first column in place of the zero border change stored elements on EVERY such 3x3 case -- channel 0 selects the
    # last input channel at the left tap of the middle filter row.  (A 1x1 case has no border to get wrong.)
    for case in F8_CASES:
        L = R.launches(case, R.SELECT)["f"]
        ref = R.conv_reference(L)["stored"]
        for mut in ("kslice", "tapshift"):
            n = int((R.conv_reference(L, mut=mut)["stored"] != ref).sum())
            assert n or (mut == "tapshift" and case.ks == 1), f"{R.case_id(case)}-{R.SELECT}: {mut} stores what the reference stores"


# ---------------------------------------------------------------------------------------------------------------------------------
# pmoe_mlp_wgrad: the reference, its generator, its mutants, and every refusal of the entry point

WG_IDS = ["-".join(str(int(v)) for v in c) for c in R.MLP_WGRAD_CASES]


def test_mlp_wgrad_reference_matches_autograd():
    E, ipe, cin, cout = 3, 5, 7, 4
    g = torch.Generator().manual_seed(23)
    x, dy = torch.randn(E * ipe, cin + 3, generator=g, dtype=F64), torch.randn(E * ipe, cout + 5, generator=g, dtype=F64)
    w, b = torch.zeros(E, cout, cin, dtype=F64, requires_grad=True), torch.zeros(E, cout, dtype=F64, requires_grad=True)
    torch.cat([F.linear(x[e * ipe:(e + 1) * ipe, 2:2 + cin], w[e], b[e]) for e in range(E)]).backward(dy[:, 1:1 + cout])
    r = R.mlp_wgrad(x, dy, cin=cin + 1, cout=cout + 1, cin_real=cin, cout_real=cout, ipe=ipe, x_coff=2, dy_coff=1)
    assert relerr(r["grads"], w.grad) < 1e-12 and relerr(r["bias_grads"], b.grad) < 1e-12
    w2 = torch.zeros(E, cout, cin, dtype=F64, requires_grad=True)
    torch.cat([F.linear(x[:ipe, 2:2 + cin], w2[e]) for e in range(E)]).backward(dy[:, 1:1 + cout])
    rs = R.mlp_wgrad(x[:ipe], dy, cin=cin + 1, cout=cout + 1, cin_real=cin, cout_real=cout, ipe=ipe, x_shared=True, x_coff=2, dy_coff=1)
    assert relerr(rs["grads"], w2.grad) < 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.MLP_WGRAD_CASES, ids=WG_IDS)
def test_mlp_wgrad_generator_properties(case, kind):
    E, ipe, cin, cin_real, cout, cout_real, shared, xc, dc = case
    d = R.mlp_wgrad_data(case, kind)
    for t, c, c_real, coff in ((d["x"], cin, cin_real, xc), (d["dy"], cout, cout_real, dc)):
        assert _representable(t, BF16)
        outside = torch.ones(t.shape[1], dtype=torch.bool)
        outside[coff:coff + c] = False
        assert torch.isnan(t[:, outside]).all() and not torch.isnan(t[:, ~outside]).any()
        assert (t[:, coff + c_real:coff + c].abs() == R.PAD_FILL).all() and t[:, coff:coff + c_real].abs().max() <= 7
        assert ipe * R.PAD_FILL ** 2 < 3e38, "sums over the pad channels stay finite in float32"
    ref = R.mlp_wgrad(d["x"], d["dy"], **d["kw"])
    assert ipe * 49 < 2 ** 24
    for reverse in (False, True):
        r32 = R.mlp_wgrad(d["x"], d["dy"], evaluate=F32, reverse=reverse, **d["kw"])
        assert torch.equal(r32["grads"].to(F64), ref["grads"]) and torch.equal(r32["bias_grads"].to(F64), ref["bias_grads"])
    assert ref["grads"].abs().max() > 0 and (kind == "unit" or ipe < 7 or ref["grads"].abs().max() > 49)


def test_every_mlp_wgrad_mutant_is_told_apart():
    for mut in R.WGRAD_MUTANTS:
        caught = []
        for case in R.MLP_WGRAD_CASES:
            for kind in R.KINDS:
                d = R.mlp_wgrad_data(case, kind)
                ref, m = R.mlp_wgrad(d["x"], d["dy"], **d["kw"]), R.mlp_wgrad(d["x"], d["dy"], mut=mut, **d["kw"])
                if not (torch.equal(ref["grads"], m["grads"]) and torch.equal(ref["bias_grads"], m["bias_grads"])):
                    caught.append((case, kind))
        assert caught, mut


# pmoe_mlp_wgrad(x, dy, grads, bias_grads, n, ipe, x_shared, cin, cout, cin_real, cout_real, x_ld, x_coff, dy_ld, dy_coff, dtype,
# stream): one accepted argument list (made-up pointers: a refused call dereferences nothing and launches nothing) and the single
# change that trips each `return PMOE_ERR_*` of pmoe_mlp_wgrad and mlp_wgrad_launch (csrc/gemm_skinny.hip), check by check
MLP_WGRAD_OK = [0x1000, 0x2000, 0x3000, 0x4000, 8, 4, 0, 16, 16, 12, 12, 32, 8, 32, 8, hip._TORCH_DT[torch.bfloat16], None]
MLP_WGRAD_REFUSED = [
    ("x null", {0: None}, -1), ("dy null", {1: None}, -1), ("grads null", {2: None}, -1),
    ("ipe 0", {5: 0}, -1), ("ipe negative", {5: -4}, -1), ("n no multiple of ipe", {4: 9}, -1),
    ("cin % 8", {7: 12}, -1), ("cout % 8", {8: 12}, -1), ("x_ld % 8", {11: 36}, -1), ("x_coff % 8", {12: 4}, -1),
    ("dy_ld % 8", {13: 36}, -1), ("dy_coff % 8", {14: 4}, -1),
    ("x window overhangs", {12: 24}, -1), ("dy window overhangs", {14: 24}, -1),
    ("cin_real 0", {9: 0}, -1), ("cin_real > cin", {9: 17}, -1), ("cout_real 0", {10: 0}, -1), ("cout_real > cout", {10: 17}, -1),
    ("float32 rows", {15: hip._TORCH_DT[torch.float32]}, -2), ("unknown dtype", {15: 7}, -2),
]


@pytest.mark.parametrize("what,change,code", MLP_WGRAD_REFUSED, ids=[r[0].replace(" ", "_") for r in MLP_WGRAD_REFUSED])
def test_mlp_wgrad_refusals(what, change, code):
    args = list(MLP_WGRAD_OK)
    for i, v in change.items():
        args[i] = v
    assert hip.load().pmoe_mlp_wgrad(*args) == code, what
