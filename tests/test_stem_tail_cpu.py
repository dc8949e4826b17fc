"""The float64 stem-tail reference (tests/stem_tail_ref.py) checked against torch's own BatchNorm/ReLU/MaxPool chain and its
autograd, and the two input generators checked for everything tests/test_stem_tail_gpu.py assumes of them.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import stem_tail_ref as R

F64 = torch.float64
IDS = [R.case_id(c) for c in R.CASES]


def _train_case():
    """float64 data whose constants ARE its batch statistics, as the engine computes them in train mode"""
    g = torch.Generator().manual_seed(3)
    E, B, H, W, C, eps = 2, 2, 9, 7, 8, 1e-5
    N = E * B
    z = torch.randn(N, H, W, C, generator=g, dtype=F64)
    dpool = torch.randn(N, R.out_size(H), R.out_size(W), C, generator=g, dtype=F64)
    g2, b2, g1 = (torch.rand(E, C, generator=g, dtype=F64) + 0.5 for _ in range(3))
    b2 = b2 - 1.0
    b1 = -torch.rand(E, C, generator=g, dtype=F64) * 0.2       # bn1(a2 == 0) < 0: plateaus of a2 tie at a3 == 0 only
    k = {}
    ze = z.reshape(E, -1, C)
    k["mu2"] = ze.mean(1)
    k["is2"] = 1 / torch.sqrt(ze.var(1, unbiased=False) + eps)
    k["sc2"], k["sh2"] = g2 * k["is2"], b2
    a2 = R.chain(z, k, B)["a2"].reshape(E, -1, C)
    k["mu1"] = a2.mean(1)
    k["is1"] = 1 / torch.sqrt(a2.var(1, unbiased=False) + eps)
    k["sc1"], k["sh1"] = g1 * k["is1"], b1
    return dict(E=E, B=B, H=H, W=W, C=C, eps=eps, z=z, dpool=dpool, k=k, g2=g2, b2=b2, g1=g1, b1=b1, count=B * H * W)


def _relerr(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_reference_matches_torch_chain_and_autograd_in_train_mode():
    t = _train_case()
    E, B, k, z, dpool, count = t["E"], t["B"], t["k"], t["z"], t["dpool"], t["count"]
    po = R.pool(z, k["sc2"], k["sh2"], k["sc1"], k["sh1"], k["mu2"], k["mu1"], B, F64)
    # no ties: a window's maximum is reached once, or it is the zero plateau (whose gradient the ReLU stops either way)
    hits = (po["cand"] == po["y"][None]).sum(0)
    assert ((hits == 1) | (po["y"] == 0)).all()
    zero = torch.zeros(E, t["C"], dtype=F64)
    k.update(c11=zero, c21=zero, c12=zero, c22=zero)
    p1 = R.bwd(1, z, dpool, po["code"], k, B)
    k["c11"], k["c21"] = p1["s1"] / count, p1["s2"] / count
    p2 = R.bwd(2, z, dpool, po["code"], k, B)
    k["c12"], k["c22"] = p2["s1"] / count, p2["s2"] / count
    dz = R.bwd(3, z, dpool, po["code"], k, B)["dz2"]
    for e in range(E):
        x = z[e * B:(e + 1) * B].permute(0, 3, 1, 2).clone().requires_grad_(True)
        a2 = F.relu(F.batch_norm(x, None, None, t["g2"][e], t["b2"][e], training=True, eps=t["eps"]))
        a3 = F.relu(F.batch_norm(a2, None, None, t["g1"][e], t["b1"][e], training=True, eps=t["eps"]))
        y = F.max_pool2d(a3, 3, 2, 1)
        y.backward(dpool[e * B:(e + 1) * B].permute(0, 3, 1, 2))
        assert _relerr(po["y"][e * B:(e + 1) * B], y.detach().permute(0, 2, 3, 1)) < 1e-10
        assert _relerr(dz[e * B:(e + 1) * B], x.grad.permute(0, 2, 3, 1)) < 1e-10
    # the pooled pass + closed forms reproduce the two sweeps over z2
    st = R.stats(z, k["sc2"], k["sh2"], k["mu2"], B)
    part_x = torch.stack([st["x0"], st["x1"], st["x2"]], 1)[:, None]
    pl = R.pooled(po["y"], dpool, po["code"], k, E)
    cb = R.combine(pl["sums"][:, None], part_x, k, count)
    assert _relerr(cb["out1"], torch.stack([p1["s1"], p1["s2"]], 1)) < 1e-9
    assert _relerr(cb["out2"], torch.stack([p2["s1"], p2["s2"]], 1)) < 1e-9


def test_first_maximum_wins_and_bit7_marks_a_positive_a2():
    """hand-made window: the tie rule, the tap numbering and the 0x80 bit of the reference itself"""
    one = torch.ones(1, 1, dtype=F64)
    z = torch.tensor([[0., 2., 2.], [2., -1., 2.], [0., 0., 0.]], dtype=F64).view(1, 3, 3, 1)
    po = R.pool(z, one, 0 * one, one, 0 * one, 0 * one, 0 * one, 1, F64)
    # windows (oy, ox): (0,0) holds rows/cols 0..1 -> first 2 is at (0,1) = tap 3*1+2; (0,1) holds cols 1..2 -> (0,1) = tap 3*1+0
    assert po["code"].view(2, 2).tolist() == [[0x80 | 5, 0x80 | 3], [0x80 | 1, 0x80 | 1]]
    assert po["y"].view(2, 2).tolist() == [[2., 2.], [2., 2.]]
    z0 = torch.zeros(1, 3, 3, 1, dtype=F64)
    po = R.pool(z0, one, 0 * one, one, 0 * one, 0 * one, 0 * one, 1, F64)
    assert po["code"].view(2, 2).tolist() == [[4, 3], [1, 0]]                # all-way tie at 0, a2 == 0: first VALID tap, bit 7 clear


def _lattice_tensors(case):
    """every intermediate of every kernel on the lattice data, and every summed term"""
    E, B, H, W, C, dtype = case
    d = R.lattice_case(case)
    z, dpool, k = d["z"], d["dpool"], d["k"]
    po = R.pool(z, k["sc2"], k["sh2"], k["sc1"], k["sh1"], k["mu2"], k["mu1"], B, dtype)
    st = R.stats(z, k["sc2"], k["sh2"], k["mu2"], B)
    p1, p2, p3 = (R.bwd(ph, z, dpool, po["code"], k, B) for ph in (1, 2, 3))
    pl = R.pooled(po["y"], dpool, po["code"], k, E)
    ch = p3["chain"]
    inter = {"u": ch["u"], "a2": ch["a2"], "a3": ch["p3"], "d1": ch["d1"], "xhat1": p3["xhat1"], "xhat2": p3["xhat2"],
             "g3": p3["g3"], "g2": p3["g2"], "xhat1P": p3["xhat1P"], "xhat2R": p3["xhat2R"], "dz2": p3["dz2"],
             "pooled_da": pl["da"], "pooled_u": pl["u"], "shiftc": st["shiftc"]}
    sums = {}
    for name, r in (("stats", st), ("phase1", p1), ("phase2", p2)):
        for tn, tt in r["terms"].items():
            sums[f"{name}.{tn}"] = tt
    for i, tt in enumerate(pl["terms"]):
        sums[f"pooled.{i}"] = tt
    return inter, sums, po, p3


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_lattice_inputs_make_float32_arithmetic_exact(case):
    E, B, H, W, C, dtype = case
    inter, sums, po, p3 = _lattice_tensors(case)
    scale = 2.0 ** R.LATTICE_G
    for name, t in {**inter, **sums}.items():
        s = t * scale
        assert (s == s.round()).all(), f"{name}: not a multiple of 2^-{R.LATTICE_G}"
        assert s.abs().max() < 2 ** 24, f"{name}: {s.abs().max().item()} lattice units"
    for name, t in sums.items():                       # an accumulator never holds more than its (expert, channel)'s absolute sum
        assert (R.esum(t.abs(), E) * scale).max() < 2 ** 24, name
    # storage: a3 and dz2 are exact in float32; where bfloat16 cannot hold them the reference rounds to nearest-even like pack16
    assert torch.equal(inter["a3"].to(torch.float32).to(F64), inter["a3"])
    assert torch.equal(inter["dz2"].to(torch.float32).to(F64), inter["dz2"])
    assert torch.equal(po["a3"], inter["a3"].clamp_min(0).to(torch.float32).to(dtype).to(F64))
    # the properties the data is meant to have: ties, plateaus, a2 == 0 and the all-way tie channel
    hits = (po["cand"] == po["y"][None]).sum(0)
    if H * W >= 64:                                   # (a 1x1 image has one candidate per window)
        assert (hits > 1).float().mean() > 0.05 and (inter["a2"] == 0).float().mean() > 0.05
    zc = R.ZERO_SC1_CHANNEL
    assert (po["y"][..., zc] == 0.5).all()
    first_valid = torch.where(po["cand"][..., zc] > -1, torch.arange(9).view(9, 1, 1, 1), 9).min(0).values
    assert torch.equal(po["tap"][..., zc], first_valid)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_continuous_inputs_keep_ambiguous_outputs_under_the_cap(case):
    d = R.continuous_case(case)
    amb = R.ambiguous_outputs(case, d)
    assert amb["outputs"].float().mean().item() <= 0.002
    # the sums and dz2 take every element: none of them may sit on a ReLU edge
    assert not R.relu_ambiguous(amb["pool"]["chain"]).any()
    # ... nor may a sum's terms be beyond what float32 can deliver of them (the premise of the sums' bound)
    assert R.term_error_share(case, d["z"], d["dpool"], d["k"]).max().item() <= R.TERM_ERROR_BUDGET
    dt = case[5]
    assert torch.equal(d["z"].to(dt).to(F64), d["z"]) and torch.equal(d["dpool"].to(dt).to(F64), d["dpool"])
