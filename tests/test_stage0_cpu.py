"""Stage 0 (trainer/train_0.py) without a GPU: the public surface exists, the container keeps the reference's state_dict
contract, ``init_weights`` reproduces the reference initializer bit for bit, and the CPU oracle restates the reference's
U-Net + stage-0 criterion (goldens of tools/make_stage0_golden.py)."""
import pytest
import torch

from oracle import pmoe_oracle as O
from oracle import weights as W
from tests import stage0_util as S
from tests.parity_util import GOLDEN


def _load(name):
    return torch.load(GOLDEN / f"{name}.pt", weights_only=False)


def test_stage0_surface_imports():
    from pmoe_amd.loss import cross_entropy_tversky_weighted_loss, dice_score
    from pmoe_amd.model.blocks import UNet
    from pmoe_amd.utils import init_weights
    assert callable(cross_entropy_tversky_weighted_loss) and callable(dice_score) and callable(init_weights("normal"))
    assert UNet.forward is not torch.nn.Module.forward and hasattr(UNet, "enable_data_parallel")


def test_unet_with_dropout_keeps_the_reference_state_dict():
    from pmoe_amd.model.blocks import UNet
    g = _load("u1_stage0_b3_32")
    m = UNet(in_features=3, out_features=23, gamma=2, b=1, dropout=0.2, inter_repr=False)
    sd = m.state_dict()
    assert list(sd.keys()) == g["state_dict_keys"]
    assert [tuple(v.shape) for v in sd.values()] == g["state_dict_shapes"]
    assert m.dropout.p == 0.2 and all(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        UNet(dropout=1.5)
    import copy
    assert list(copy.deepcopy(m).state_dict().keys()) == g["state_dict_keys"]


def test_init_weights_equals_the_reference_initializer():
    """same seed, same module order -> the same draws from torch's generator: torch.equal on every stored digest value"""
    from pmoe_amd.model.blocks import UNet
    from pmoe_amd.utils import init_weights
    g = _load("u0_init")
    assert g["seed"] == S.INIT_SEED
    torch.manual_seed(0)
    got = S.init_digests(UNet(dropout=0.1), lambda m: init_weights(method=m))
    assert set(got) == set(g["digests"]) == {m for m, _ in S.INIT_METHODS}
    for method, ref in g["digests"].items():
        assert got[method].keys() == ref.keys(), method
        for k in ref:
            assert S.digests_equal(got[method][k], ref[k]), (method, k, got[method][k], ref[k])
    assert g["digests"]["xavier_normal"]["raises"] == "ValueError"
    # ConvTranspose2d is not in the reference's isinstance lists: untouched; biases are zeroed where present
    m = UNet()
    before = m.up_1.weight.detach().clone()
    m.apply(init_weights("uniform", low=2.0, high=3.0))
    assert torch.equal(m.up_1.weight, before) and m.out.bias.abs().max().item() == 0.0
    assert m.dwn_1[1].weight.min().item() >= 2.0 and m.dwn_1[0].weight.min().item() >= 2.0
    with pytest.raises(ValueError):
        init_weights("kaiming_uniform")          # the reference spells it with a trailing underscore


@pytest.mark.parametrize("name", ["u1_stage0_b3_32", "u2_stage0_b8_64"])
def test_oracle_restates_the_reference_stage0_step(name):
    g = _load(name)
    net = O.UNet()
    assert list(net.state_dict().keys()) == g["state_dict_keys"]
    W.fill_state_dict(net, seed=g["meta"]["weight_seed"])
    net.train()
    image, target = S.case_inputs(g["meta"])
    out = net(image)
    out.retain_grad()
    loss = O.cross_entropy_tversky_weighted_loss(out, target)
    loss.backward()
    torch.testing.assert_close(out.detach()[..., ::4, ::4], g["out_sub"], rtol=1e-5, atol=1e-6)
    assert out.detach().norm().item() == pytest.approx(g["out_norm"], rel=1e-5)
    torch.testing.assert_close(loss.detach(), g["loss"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out.grad[..., ::4, ::4], g["dout_sub"], rtol=1e-4, atol=1e-6 * g["dout_sub"].abs().max().item())
    named = dict(net.named_parameters())
    assert set(named) == set(g["grad_norms"])
    for k, n in g["grad_norms"].items():
        assert named[k].grad.norm().item() == pytest.approx(n, rel=1e-4, abs=1e-7), k
    for k, sl in g["grad_slices"].items():
        torch.testing.assert_close(named[k].grad.flatten()[:64], sl, rtol=1e-4, atol=1e-6)
    sd = net.state_dict()
    for k, v in g["bn_after_1"].items():
        torch.testing.assert_close(sd[k], v, rtol=1e-5, atol=1e-6)


def test_oracle_restates_the_reference_metrics():
    for nm, c in _load("u0_metrics").items():
        x = c["logits"].clone().requires_grad_(True)
        loss = O.cross_entropy_tversky_weighted_loss(x, c["target"], *c["weights"])
        loss.backward()
        torch.testing.assert_close(loss.detach(), c["loss"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(x.grad, c["dlogits"], rtol=1e-4, atol=1e-9)
        torch.testing.assert_close(S.dice_oracle(c["logits"], c["target"]), c["dice"], rtol=1e-6, atol=0)


def test_stage0_loss_rejects_weights_that_do_not_sum_to_one():
    from pmoe_amd.loss import cross_entropy_tversky_weighted_loss
    x, t = torch.zeros(1, 23, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="sum to 1"):
        cross_entropy_tversky_weighted_loss(x, t, 0.5, 0.6)
    with pytest.raises(ValueError):
        cross_entropy_tversky_weighted_loss(x, t.int())
    with pytest.raises(ValueError):
        cross_entropy_tversky_weighted_loss(x[0], t)


def test_stage0_has_no_cpu_path():
    from pmoe_amd.model.blocks import UNet
    with pytest.raises(RuntimeError, match="no CPU path"):
        UNet()(torch.zeros(1, 3, 16, 16))
