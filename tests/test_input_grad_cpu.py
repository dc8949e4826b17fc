"""tests/input_grad_ref.py against torch.autograd in float64, and the exactness condition of its lattice generators."""
import pytest
import torch

from tests import input_grad_ref as R

F64 = torch.float64


@pytest.mark.parametrize("E,B,H,W,C,k", [(1, 1, 6, 7, 3, 1), (3, 2, 5, 9, 12, 3), (2, 2, 16, 16, 12, 5)])
def test_stem_restatement_is_autograd(E, B, H, W, C, k):
    """d/dx of sum_e <dz1_e, conv2d(x * sigmoid(conv1d(gap(x))), W_e)> for E independent experts that share x"""
    g = torch.Generator().manual_seed(11 * E + H)
    Co = 8
    x = torch.randn(B, C, H, W, generator=g, dtype=F64)
    w = torch.randn(E, Co, C, 3, 3, generator=g, dtype=F64) / 4
    w1d = torch.randn(E, k, generator=g, dtype=F64)
    dz1 = torch.randn(E, B, H, W, Co, generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    total = 0
    for e in range(E):
        y = torch.nn.functional.adaptive_avg_pool2d(xr, 1)
        y = torch.nn.functional.conv1d(y.squeeze(-1).transpose(-1, -2), w1d[e].view(1, 1, k), padding=k // 2)
        y = torch.sigmoid(y.transpose(-1, -2).unsqueeze(-1))
        z1 = torch.nn.functional.conv2d(xr * y.expand_as(xr), w[e], stride=1, padding=1)
        total = total + (z1 * dz1[e].permute(0, 3, 1, 2)).sum()
    total.backward()
    gate, _ = R.gate_of(x, w1d)
    dgap = R.dgap_of(x, w, w1d, gate, dz1)
    got = R.stem_input_grad(dz1, R.gated(w, gate), dgap / (H * W))
    assert got.shape == x.shape
    assert (got - xr.grad).abs().max().item() <= 1e-12 * xr.grad.abs().max().item()
    # without the gate term the restatement is the plain transposed convolution of the gated weights
    plain = R.stem_input_grad(dz1, R.gated(w, gate))
    assert (plain - xr.grad).abs().max().item() > 1e-6 * xr.grad.abs().max().item()


@pytest.mark.parametrize("E,B,O,J", [(1, 1, 5, 1), (3, 4, 20, 6)])
def test_shared_linear_restatement_is_autograd(E, B, O, J):
    g = torch.Generator().manual_seed(O)
    x = torch.randn(B, J, generator=g, dtype=F64, requires_grad=True)
    wl = torch.randn(E, O, J, generator=g, dtype=F64)
    dh = torch.randn(E, B, O, generator=g, dtype=F64)
    sum((torch.nn.functional.linear(x, wl[e]) * dh[e]).sum() for e in range(E)).backward()
    got = R.shared_linear_input_grad(dh, wl)
    assert (got - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_lattice_partial_sums_stay_exact(shape):
    """every operand a multiple of its unit and exact in bf16, every partial sum (in any order) below 2^24 lattice units"""
    d = R.lattice_stem(7, *shape)
    wg = R.gated(d["w"], d["gate"])
    for t, unit in ((d["dz1"], 1 / 4), (wg, 1 / 32), (d["dgap_hw"], 1 / 8)):
        assert torch.equal(t / unit, (t / unit).round())
        assert torch.equal(t.to(torch.bfloat16).to(F64), t)
    assert R.largest_partial_sum(d) < 2 ** 24
    assert R.stem_terms(shape[0]) * 1.75 / R.LATTICE_UNIT + 3 * 2 * 128 < 2 ** 24          # (the a-priori form of the same bound)


@pytest.mark.parametrize("shape", R.LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_lattice_partial_sums_stay_exact(shape):
    d = R.lattice_linear(7, *shape)
    for t in d.values():
        assert torch.equal(t.to(torch.bfloat16).to(F64), t)
    assert R.shared_linear_input_grad(d["dh"], d["wl"], absolute=True).max().item() * 32 < 2 ** 24
