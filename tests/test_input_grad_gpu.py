"""Input gradients (-m gpu): pmoe_stem_input_grad and pmoe_shared_linear_input_grad against tests/input_grad_ref.py through
``ops``, then ``images.grad`` / ``speed.grad`` / ``command.grad`` of the drop-in modules against the float64 oracle evaluated on
the HIP path's own decisions (tests/forced_masks.py), the launch plan of such a backward, and the bf16 kernel on a model's own
operands.

Bounds.  Lattice data (input_grad_ref.lattice_*): bit-equal to float64, whatever the summation order.  Random data: the
kernels sum K exact-or-once-rounded products in f32, so |got - ref| <= (K + 2) 2^-24 sum|terms| per element (K = E * 9 * 64 for
the stem, E * cout for the Linear; the + 2: the gate-term sum and its addition).  Model level, f32: rel-L2 at
parity_util.FORCED_GRAD_TOL (10 x for tensors of fewer than 64 elements, as there)."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

from pmoe_amd import hip, ops  # noqa: E402
from tests import input_grad_ref as R  # noqa: E402

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SENTINEL = -77.0
GUARD = 64


def _guarded(shape, lead):
    """an f32 tensor of ``shape`` inside a sentinel-filled buffer, ``lead`` floats from its start -> (view, buffer)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=F32, device=DEV)
    return buf[lead:lead + n].view(shape), buf


def _guards_intact(buf, lead):
    return bool((buf[:lead] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _stem_operands(d, dtype, C):
    """lattice / random data of input_grad_ref -> (dz1 [E*B,H,W,64], wd pack, dgap [E*B,16], wg as stored, dz1 as stored)"""
    E, B, H, W, Co = d["dz1"].shape
    N = E * B
    dz1 = d["dz1"].reshape(N, H, W, Co).to(dtype).to(DEV).contiguous()
    ws = [d["w"][e].to(F32).to(DEV).contiguous() for e in range(E)]
    gate = torch.zeros(N, 16, dtype=F32, device=DEV)
    gate[:, :C] = d["gate"].reshape(N, C).to(F32).to(DEV)
    gate[:, C:] = 3.0                                   # (channels past the real ones: the pack must write zeros there)
    wd = torch.full((N, 64, 9, 64), 5.0, dtype=dtype, device=DEV)
    ops.pack_conv_weights_gated(hip.ptr_table(ws, DEV), gate, None, wd, N, B, Co, C, 3, 64, 16, 64, 64, dtype)
    dgap = torch.full((N, 16), 9.0, dtype=F32, device=DEV)          # (columns past C: read, never stored)
    dgap[:, :C] = d["dgap_hw"].reshape(N, C).to(F32).to(DEV)
    # what the kernel reads: wd[n][c][8 - t][co] = wg[n][co][c][t]
    wg = wd[:, :C].flip(2).permute(0, 3, 1, 2).reshape(E, B, Co, C, 3, 3).to(F64)
    assert not wd[:, C:].any()
    return dz1, wd, dgap, wg, dz1.view(E, B, H, W, Co).to(F64), ws


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_input_grad_kernel(shape, dtype):
    E, B, H, W, C = shape
    K = R.stem_terms(E)
    for kind, make in (("lattice", R.lattice_stem), ("random", R.random_stem)):
        d = make(3, *shape)
        dz1, wd, dgap, wg, dz64, _ws = _stem_operands(d, dtype, C)
        if kind == "lattice":
            assert torch.equal(wg.cpu(), R.gated(d["w"], d["gate"]))          # the pack holds gate * W exactly
        for with_dgap, lead in ((True, 64), (False, 65)):                       # (65: dx not 16-byte aligned)
            dx, buf = _guarded((B, C, H, W), lead)
            ops.stem_input_grad(dz1, wd, dgap if with_dgap else None, dx, E)
            got = dx.clone()
            dg64 = dgap[:, :C].view(E, B, C).to(F64) if with_dgap else None
            ref = R.stem_input_grad(dz64, wg, dg64)
            assert _guards_intact(buf, lead), (kind, with_dgap)
            assert not (got == SENTINEL).any()
            if kind == "lattice":
                assert torch.equal(got.to(F64), ref), (kind, with_dgap, (got.to(F64) - ref).abs().max().item())
            else:
                bound = (K + 2) * R.EPS24 * R.stem_input_grad(dz64, wg, dg64, absolute=True)
                worst = ((got.to(F64) - ref).abs() / bound).max().item()
                print(f"stem {shape} {dtype} dgap={with_dgap}: worst error {worst:.3f} of the bound")
                assert worst <= 1.0, (kind, with_dgap, worst)
            dx.fill_(SENTINEL)
            ops.stem_input_grad(dz1, wd, dgap if with_dgap else None, dx, E)
            assert torch.equal(dx, got)
    torch.cuda.synchronize()


def test_stem_input_grad_refuses_bad_operands():
    dz1 = torch.zeros(2, 16, 16, 64, dtype=BF16, device=DEV)
    wd = torch.zeros(2, 64, 9, 64, dtype=BF16, device=DEV)
    dx = torch.zeros(1, 12, 16, 16, dtype=F32, device=DEV)
    with pytest.raises(ValueError):
        ops.stem_input_grad(dz1, wd, None, torch.zeros(1, 17, 16, 16, dtype=F32, device=DEV), 2)       # more than 16 channels
    with pytest.raises(ValueError):
        ops.stem_input_grad(dz1, wd, None, torch.zeros(1, 12, 16, 15, dtype=F32, device=DEV), 2)       # another map
    with pytest.raises(ValueError):
        ops.stem_input_grad(dz1, wd[:, :8].contiguous(), None, dx, 2)                                  # a pack of 8 channel rows
    with pytest.raises(ValueError):
        ops.stem_input_grad(dz1, wd, torch.zeros(2, 12, dtype=F32, device=DEV), dx, 2)                 # dgap rows of 12
    with pytest.raises(ValueError):
        ops.stem_input_grad(dz1, wd.float(), None, dx, 2)                                              # pack of another dtype
    assert hip.load().pmoe_stem_input_grad(None, None, None, None, 1, 1, 16, 16, 12, 64, 64, 0, None) == hip.ERR_ARG


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", R.LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shared_linear_input_grad_kernel(shape, dtype):
    E, B, O, J = shape
    coutp, cinp = (O + 63) // 64 * 64, 16
    for kind, make in (("lattice", R.lattice_linear), ("random", R.random_linear)):
        d = make(5, *shape)
        for ld, coff in (((O + 15) // 16 * 16, 0), (1536, 512)):                # dense rows | a window of the 1536-wide feature
            dh = torch.full((E * B, 1, 1, ld), 7.0, dtype=dtype, device=DEV)
            dh[..., coff:coff + O] = d["dh"].reshape(E * B, 1, 1, O).to(dtype).to(DEV)
            w = torch.full((E, coutp, 1, cinp), 7.0, dtype=dtype, device=DEV)   # (rows / columns past the real ones: never read)
            w[:, :O, 0, :J] = d["wl"].to(dtype).to(DEV)
            dh64 = dh[..., coff:coff + O].reshape(E, B, O).to(F64)
            w64 = w[:, :O, 0, :J].to(F64)
            dx, buf = _guarded((B, J), 64)
            ops.shared_linear_input_grad(dh, w, dx, E, O, dh_coff=coff)
            got = dx.clone()
            ref = R.shared_linear_input_grad(dh64, w64)
            assert _guards_intact(buf, 64)
            if kind == "lattice":
                assert torch.equal(got.to(F64), ref)
            else:
                bound = (E * O + 2) * R.EPS24 * R.shared_linear_input_grad(dh64, w64, absolute=True)
                assert ((got.to(F64) - ref).abs() <= bound).all()
            dx.fill_(SENTINEL)
            ops.shared_linear_input_grad(dh, w, dx, E, O, dh_coff=coff)
            assert torch.equal(dx, got)
    with pytest.raises(ValueError):
        ops.shared_linear_input_grad(dh, w, torch.zeros(B + 1, J, dtype=F32, device=DEV), E, O, dh_coff=coff)
    with pytest.raises(ValueError):
        ops.shared_linear_input_grad(dh, w, dx, E, O, dh_coff=ld - O + 1)


# ------------------------------------------------------------------------------------------------ model level
def _leaves(inp, dev, cast=lambda t: t, names=("images", "speed", "command")):
    out = {k: cast(v).to(dev) for k, v in inp.items()}
    for k in names:
        out[k] = out[k].detach().clone().requires_grad_(True)
    return out


def _hip_step(model, ocfg, d):
    from pmoe_amd.loss import moe_loss
    model.zero_grad(set_to_none=True)
    dist, speeds = model(d["images"], d["speed"], d["command"])
    moe_loss(dist, speeds, d["control"], d["target_speed"], ocfg.loss_coefs).backward()
    return {k: p.grad.clone() if p.grad is not None else None for k, p in model.named_parameters()}


def _check_input_grads(name, got, ref):
    from tests.parity_util import FORCED_GRAD_TOL, rel_l2
    for k, g in got.items():
        assert g is not None, f"{name}: {k}.grad is None"
        assert g.shape == ref[k].shape and torch.isfinite(g).all(), k
        e = rel_l2(g, ref[k])
        tol = FORCED_GRAD_TOL if g.numel() >= 64 else 10 * FORCED_GRAD_TOL
        print(f"{name} d loss / d {k}: rel-L2 {e:.2e} (bound {tol:g}, {g.numel()} elements)")
        assert e <= tol, (name, k, e)


def _forced_input_grads(g, ocfg, oracle, eng, inp, names):
    from oracle import pmoe_oracle as O
    from tests import forced_masks as FM
    m = g["meta"]

    def run(m64, cast):
        d = _leaves(inp, "cpu", cast, names)
        dist, s = m64(d["images"], d["speed"], d["command"])
        O.moe_loss(dist, s, d["control"], d["target_speed"].clone(), ocfg.loss_coefs).backward()
        return {k: d[k].grad for k in names}
    out, _, _ = FM.forced_float64(oracle, eng, inp, m["batch"], run, alt=m["type"] == "moe_alt", shared=m["type"] == "moe_shared")
    return out


@pytest.mark.parametrize("name", ["g4_moealt_e4_b2_64", "g5_moe_e3_b3_96", "g9_moeshared_k5_b8_64"])
def test_input_grads_match_the_forced_float64_oracle_f32(name):
    """images.grad, speed.grad and command.grad of a training step, and nothing else moves: every parameter gradient of the
    same backward is bit-equal to the one of a step that asks for no input gradient (the f32 path has no deferral to give up)"""
    from tests.parity_util import GOLDEN, build_pair
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    ocfg, oracle, model, inp = build_pair(g, F32)
    plain = _hip_step(model, ocfg, {k: v.to(DEV) for k, v in inp.items()})
    eng = model._engine()
    eng.debug_acts = {}
    d = _leaves(inp, DEV)
    with_inputs = _hip_step(model, ocfg, d)
    got = {k: d[k].grad for k in ("images", "speed", "command")}
    ref = _forced_input_grads(g, ocfg, oracle, eng, inp, ("images", "speed", "command"))
    eng.debug_acts = None
    _check_input_grads(name, got, ref)
    for k, p in plain.items():
        assert p is not None and torch.equal(p, with_inputs[k]), k


def test_saliency_of_a_frozen_eval_model_f32():
    """eval mode, every parameter frozen, only images.requires_grad: the gradient arrives, matches the float64 oracle in eval
    mode, and no parameter gets a .grad"""
    from tests.parity_util import GOLDEN, build_pair
    name = "g5_moe_e3_b3_96"
    g = torch.load(GOLDEN / f"{name}.pt", weights_only=False)
    ocfg, oracle, model, inp = build_pair(g, F32)
    model.eval()
    oracle.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    eng = model._engine()
    eng.debug_acts = {}
    d = _leaves(inp, DEV, names=("images",))
    _hip_step(model, ocfg, d)
    assert d["speed"].grad is None and d["command"].grad is None
    ref = _forced_input_grads(g, ocfg, oracle, eng, inp, ("images",))
    eng.debug_acts = None
    _check_input_grads(name + " eval, frozen", {"images": d["images"].grad}, ref)
    assert all(p.grad is None for p in model.parameters())
    # and under no_grad nothing is taped or returned
    with torch.no_grad():
        dist, _ = model(d["images"], d["speed"], d["command"])
    assert not dist.hip_params[0].requires_grad


def test_lone_expert_and_speed_only():
    """a BaseExpert called on its own (group of one), and a call in which only ``speed`` asks: each gets its gradient, the
    others stay None"""
    from oracle import weights as W
    from pmoe_amd.model.moe import BaseExpert
    from pmoe_amd.utils import stage2_model_cfg
    model = W.fill_state_dict(BaseExpert(stage2_model_cfg("moe", 2, dropout=0.0)), seed=3).to(DEV)
    model.compute_dtype = F32
    inp = W.make_inputs(2, 64, 64, seed=5)
    d = _leaves(inp, DEV)
    alpha, mean, std, sp = model(d["images"], d["speed"], d["command"])
    (alpha.sum() + mean.square().sum() + std.sum() + sp.sum()).backward()
    for k in ("images", "speed", "command"):
        assert d[k].grad is not None and d[k].grad.shape == d[k].shape and d[k].grad.abs().sum() > 0, k
    d = _leaves(inp, DEV, names=("speed",))
    alpha, mean, std, sp = model(d["images"], d["speed"], d["command"])
    (mean.square().sum() + sp.sum()).backward()
    assert d["speed"].grad is not None and d["images"].grad is None and d["command"].grad is None


def test_launch_plan_of_a_backward_with_input_gradients():
    """one stem-input-gradient launch (+ its gated pack), one launch each for speed and command, no layout pass, no ECA apply
    pass and no data-gradient convolution of conv1 -- and in f32, where nothing is deferred, nothing else changes"""
    from tests import launch_seq as LS
    from tests.parity_util import GOLDEN, build_pair
    g = torch.load(GOLDEN / "g5_moe_e3_b3_96.pt", weights_only=False)
    for dtype in (F32, BF16):
        ocfg, _, model, inp = build_pair(g, dtype)
        seqs = {}
        for which, names in (("plain", ()), ("inputs", ("images", "speed", "command"))):
            d = _leaves(inp, DEV, names=names)
            _hip_step(model, ocfg, d)                     # (first-use packs and planning calls out of the way)
            with hip.LaunchRecorder() as rec:
                _hip_step(model, ocfg, d)
            torch.cuda.synchronize()
            seqs[which] = LS.reduce_calls(rec.calls)
        names = {k: collections.Counter(r[0] for r in v) for k, v in seqs.items()}
        assert names["inputs"]["pmoe_stem_input_grad"] == 1 and names["plain"]["pmoe_stem_input_grad"] == 0
        assert names["inputs"]["pmoe_shared_linear_input_grad"] == 2
        for absent in ("pmoe_nhwc_to_nchw", "pmoe_eca_bwd_apply"):
            assert names["inputs"][absent] == 0, absent
        conv1_dgrad = [r for r in seqs["inputs"] if r[0] == "pmoe_conv2d_igemm" and LS.field(r, "ks") == 3
                       and LS.field(r, "cout") == 16 and LS.field(r, "cin") == 64]
        assert not conv1_dgrad
        if dtype == F32:
            assert names["inputs"] - names["plain"] == collections.Counter(
                {"pmoe_stem_input_grad": 1, "pmoe_pack_conv_weights_gated": 1, "pmoe_shared_linear_input_grad": 2})
            assert not names["plain"] - names["inputs"]


def test_bf16_kernel_on_a_models_own_operands():
    """g10 (E=4, B=32, 64 x 64), bf16: the launch's actual dz1, packs and dgap through ``debug_input_grad`` against the float64
    restatement evaluated on those same tensors, at the derived bound.  The end-to-end distance of the bf16 image gradient from
    the f32 path's is printed only: it is the storage format's, not derivable (DESIGN.md section 2 records it)."""
    from tests.parity_util import GOLDEN, build_pair, rel_l2
    g = torch.load(GOLDEN / "g10_moe_e4_b32_64.pt", weights_only=False)
    ocfg, _, model, inp = build_pair(g, BF16)
    eng = model._engine()
    eng.debug_input_grad = {}
    d = _leaves(inp, DEV, names=("images",))
    _hip_step(model, ocfg, d)
    k = eng.debug_input_grad
    eng.debug_input_grad = None
    E, B = 4, 32
    N, H, W, Co = k["dz1"].shape
    C = d["images"].shape[1] * d["images"].shape[2]
    assert (N, H, W, Co) == (E * B, 64, 64, 64) and k["dz1"].dtype == BF16 and k["wd"].dtype == BF16
    wg = k["wd"][:, :C].flip(2).permute(0, 3, 1, 2).reshape(E, B, Co, C, 3, 3)
    dz64, dg64 = k["dz1"].view(E, B, H, W, Co), k["dgap"][:, :C].view(E, B, C)
    ref = R.stem_input_grad(dz64, wg, dg64)
    bound = (R.stem_terms(E) + 2) * R.EPS24 * R.stem_input_grad(dz64, wg, dg64, absolute=True)
    got = d["images"].grad.view(B, C, H, W)
    assert torch.equal(got, k["dx"])
    worst = ((got.to(F64) - ref).abs() / bound).max().item()
    print(f"g10 bf16 stem input gradient on the model's operands: worst error {worst:.3f} of the bound")
    assert worst <= 1.0
    bf = got.clone()
    model.compute_dtype = F32
    d = _leaves(inp, DEV, names=("images",))
    _hip_step(model, ocfg, d)
    f = d["images"].grad.view(B, C, H, W)
    cos = torch.nn.functional.cosine_similarity(bf.flatten().double(), f.flatten().double(), dim=0).item()
    print(f"g10 d loss / d images, bf16 path vs f32 path: rel-L2 {rel_l2(bf, f):.3e}, cosine {cos:.4f} (no pass mark)")
