"""Helpers shared by the stage-0 tests (tests/test_stage0_cpu.py, tests/test_stage0_gpu.py) and the golden generator
(tools/make_stage0_golden.py): inputs, the initializer digests, and the oracle U-Net forward with Dropout2d replayed."""
import math

import torch
import torch.nn.functional as F

from oracle import pmoe_oracle as O
from oracle import weights as W

CASES = {"u1_stage0_b3_32": dict(batch=3, size=32, train=True),
         "u2_stage0_b8_64": dict(batch=8, size=64, train=True),
         "u3_stage0_b1_224_eval": dict(batch=1, size=224, train=False)}
SLICES = ["dwn_1.0.weight", "dwn_1.1.weight", "dwn_3.3.weight", "dwn_5.1.bias", "up_2.weight", "up_2.bias",
          "up_forw_4.4.weight", "out.weight", "out.bias"]
BN_LAYERS = ["dwn_1.1", "dwn_5.4", "up_forw_1.1", "up_forw_4.4"]
# (method, applies to the whole U-Net): torch's Xavier fills reject the 1-D weight of a BatchNorm, which both initializers
# match for those methods -- on the U-Net they raise ValueError, so their values are pinned on BatchNorm-free sub-modules
INIT_METHODS = [("kaiming_normal", True), ("kaiming_uniform_", True), ("normal", True), ("uniform", True),
                ("xavier_normal", False), ("xavier_uniform", False)]
INIT_SEED = 20
XAVIER_PARTS = ["dwn_1.0", "dwn_4.3", "out"]
SANITY = dict(steps=30, lr=1e-3)


def case_inputs(meta):
    """image [B,3,H,W] f32 in [0,1), target [B,H,W] int64 -- frame 0 of the shared synthetic batch."""
    image = W.make_inputs(meta["batch"], meta["size"], meta["size"], seed=meta["input_seed"])["images"][:, 0].contiguous()
    target = W.make_seg_targets(meta["batch"], 1, meta["size"], meta["size"], 23, seed=meta["target_seed"])[:, 0].contiguous()
    return image, target


def tensor_digest(t):
    """(sum, abs-sum, first 8 values) of a tensor; the sums are exactly rounded (math.fsum), i.e. independent of the
    summation order, thread count and vector width of the machine that forms them."""
    v = t.detach().double().flatten().tolist()
    return dict(sum=math.fsum(v), abs_sum=math.fsum(abs(x) for x in v), first8=t.detach().flatten()[:8].clone())


def init_digests(model, make_init, sub=lambda m, name: m.get_submodule(name)):
    """digests of ``model`` after ``model.apply(make_init(method))`` for every method, under torch.manual_seed(INIT_SEED);
    the Xavier methods on the BatchNorm-free sub-modules XAVIER_PARTS (and "raises" records that the whole model raises)."""
    out = {}
    for method, whole in INIT_METHODS:
        torch.manual_seed(INIT_SEED)
        if whole:
            model.apply(make_init(method))
            out[method] = {k: tensor_digest(v) for k, v in model.state_dict().items() if v.is_floating_point()}
            continue
        rec = {}
        for part in XAVIER_PARTS:
            m = sub(model, part)
            m.apply(make_init(method))
            rec.update({f"{part}.{k}": tensor_digest(v) for k, v in m.state_dict().items()})
        try:
            model.apply(make_init(method))
            rec["raises"] = None
        except ValueError:
            rec["raises"] = "ValueError"
        out[method] = rec
    return out


def digests_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(digests_equal(a[k], b[k]) for k in a)
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return a == b


def oracle_unet_dropout(net, image, tables):
    """``blocks/unet.py:50-95`` on the oracle U-Net's layers with Dropout2d REPLAYED: ``tables`` are the four [B,C] scale tables
    (0 or 1/(1-p)) that the HIP engine drew for x_1..x_4, so both sides drop the same feature maps."""
    skips, x = [], image
    for blk, tab in zip((net.dwn_1, net.dwn_2, net.dwn_3, net.dwn_4), tables):
        x = blk(x) * tab.to(image.dtype)[:, :, None, None]
        skips.append(x)
        x = F.max_pool2d(x, 2, 2)
    x = net.dwn_5(x)
    for up, fw in ((net.up_1, net.up_forw_1), (net.up_2, net.up_forw_2), (net.up_3, net.up_forw_3), (net.up_4, net.up_forw_4)):
        skip = skips.pop()
        x = fw(torch.cat([skip, up(x, output_size=skip.size())], 1))
    return net.out(x)


def dice_oracle(pred, target, eps=1e-6):
    """``trainer/loss.py:20-31`` restated: per-class 2 (inter + eps) / (pred + target + eps) of the arg-max prediction, f32."""
    hard = pred.argmax(dim=1)
    out = torch.ones(pred.size(1), dtype=torch.float)
    for c in range(pred.size(1)):
        p, t = hard == c, target == c
        out[c] = 2 * ((p & t).sum().float() + eps) / (p.sum() + t.sum() + eps)
    return out


# ---------------------------------------------------------------------------- golden generation (tools/make_stage0_golden.py)
def import_reference():
    """the imported reference with the stand-ins of oracle/make_golden.py -> (its loss module, UNet, init_weights); build
    machine only"""
    from oracle import make_golden
    make_golden.import_reference()
    import loss as ref_loss
    from model.blocks.unet import UNet as RefUNet
    from utils.nn import init_weights as ref_init
    return ref_loss, RefUNet, ref_init


def fill_weights(module, seed=0):
    return W.fill_state_dict(module, seed=seed)


def seg_targets(batch, height, width, classes, seed, block=2):
    return W.make_seg_targets(batch, 1, height, width, classes, seed=seed, block=block)[:, 0].contiguous()


def sanity_ratio(meta):
    """the CPU oracle's f32 loss ratio loss_30 / loss_0 for the training-sanity recipe: Adam(lr=1e-3, amsgrad) on one fixed batch"""
    net = O.UNet()
    W.fill_state_dict(net, seed=meta["weight_seed"])
    net.train()
    image, target = case_inputs(meta)
    opt = torch.optim.Adam(net.parameters(), lr=SANITY["lr"], amsgrad=True)
    losses = []
    for _ in range(SANITY["steps"] + 1):
        loss = O.cross_entropy_tversky_weighted_loss(net(image), target)
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    return dict(loss_0=losses[0], loss_n=losses[-1], ratio=losses[-1] / losses[0], steps=SANITY["steps"])
