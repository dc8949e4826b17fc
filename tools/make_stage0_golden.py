#!/usr/bin/env python3
"""Generate tests/golden/u*.pt -- the stage-0 fixtures -- by running the imported reference (its ``UNet``, ``trainer/loss.py``
and ``utils/nn.py:init_weights``).  Runs on the build machine only, where the reference tree is present; the outputs are small
data files: weights are re-derived from seeds, large tensors are sub-sampled.  Everything that touches the CPU-oracle package
(the reference import with its stand-ins, the seed-derived weights and targets, the training-sanity recipe) is test
infrastructure and lives in tests/stage0_util.py; this file only drives it.  Usage:  python tools/make_stage0_golden.py
"""
import os
import sys
from pathlib import Path

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from tests import stage0_util as S               # noqa: E402


def run_case(RefUNet, ref_loss, name, batch, size, train):
    torch.manual_seed(0)
    model = RefUNet(in_features=3, out_features=23, gamma=2, b=1, dropout=0.0, inter_repr=not train)
    S.fill_weights(model, seed=0)
    model.train(train)
    meta = dict(name=name, batch=batch, size=size, train=train, weight_seed=0, input_seed=1234, target_seed=4321)
    image, target = S.case_inputs(meta)
    sd_keys = list(model.state_dict().keys())
    res = {"meta": meta, "state_dict_keys": sd_keys,
           "state_dict_shapes": [tuple(v.shape) for v in model.state_dict().values()]}
    if not train:
        with torch.no_grad():
            inter, out = model(image)
        res.update(out_sub=out[..., ::4, ::4].clone(), out_norm=out.norm().item(), inter=inter.clone(),
                   loss=ref_loss.cross_entropy_tversky_weighted_loss(out, target).clone(),
                   dice=ref_loss.dice_score(out, target).clone())
        return res
    out = model(image)
    out.retain_grad()
    loss = ref_loss.cross_entropy_tversky_weighted_loss(out, target)
    loss.backward()
    named = dict(model.named_parameters())
    sd = model.state_dict()
    res.update({"out_sub": out.detach()[..., ::4, ::4].clone(), "out_norm": out.detach().norm().item(),
                "loss": loss.detach().clone(), "dice": ref_loss.dice_score(out.detach(), target).clone(),
                "dout_sub": out.grad[..., ::4, ::4].clone(), "dout_norm": out.grad.norm().item(),
                "grad_norms": {k: p.grad.norm().item() for k, p in named.items()},
                "grad_slices": {k: named[k].grad.flatten()[:64].clone() for k in S.SLICES},
                "bn_after_1": {f"{b}.{leaf}": sd[f"{b}.{leaf}"].clone() for b in S.BN_LAYERS
                               for leaf in ("running_mean", "running_var", "num_batches_tracked")}})
    return res


def metric_cases(ref_loss):
    """dice_score and cross_entropy_tversky_weighted_loss (loss + d loss / d logits) on random logits, on logits with exact
    arg-max ties, and with a class that neither the prediction nor the target contains."""
    g = torch.Generator().manual_seed(77)
    out = {}
    specs = {"a": (2, 23, 16, 16, 2.0, (0.5, 0.5)), "b": (3, 23, 8, 24, 0.5, (0.25, 0.75)), "c": (2, 5, 12, 20, 1.0, (0.75, 0.25))}
    for nm, (b, c, h, w, scale, wts) in specs.items():
        x = torch.randn(b, c, h, w, generator=g) * scale
        t = S.seg_targets(b, h, w, c, seed=11 + b)
        out[nm] = (x, t, wts)
    # exact ties: logits on a grid of five values -- most pixels have several maximal classes (torch.argmax: the first)
    x = torch.randint(-2, 3, (2, 23, 16, 16), generator=g).float() / 2
    out["ties"] = (x, S.seg_targets(2, 16, 16, 23, seed=5), (0.5, 0.5))
    # classes 3 and 22 absent from prediction and target: their dice is 2 eps / eps
    x = torch.randn(2, 23, 16, 16, generator=g)
    x[:, 3] = -30.0
    x[:, 22] = -30.0
    t = S.seg_targets(2, 16, 16, 23, seed=6)
    t[t == 3] = 4
    t[t == 22] = 0
    out["absent"] = (x, t, (0.5, 0.5))
    res = {}
    for nm, (x, t, wts) in out.items():
        xi = x.clone().requires_grad_(True)
        loss = ref_loss.cross_entropy_tversky_weighted_loss(xi, t, *wts)
        loss.backward()
        res[nm] = dict(logits=x.clone(), target=t, weights=wts, loss=loss.detach().clone(), dlogits=xi.grad.clone(),
                       dice=ref_loss.dice_score(x, t).clone())
    assert res["absent"]["dice"][3].item() == 2.0 and (res["ties"]["logits"].max(1)[0][:, :, :, None].eq(
        res["ties"]["logits"].movedim(1, -1)).sum(-1) > 1).float().mean() > 0.5
    return res


def main():
    ref_loss, RefUNet, ref_init = S.import_reference()
    gold = REPO / "tests" / "golden"
    for name, c in S.CASES.items():
        res = run_case(RefUNet, ref_loss, name, c["batch"], c["size"], c["train"])
        if name.startswith("u2"):
            res["meta"]["sanity"] = S.sanity_ratio(res["meta"])
            print(name, "sanity", res["meta"]["sanity"])
        torch.save(res, gold / f"{name}.pt")
        print(name, "loss", float(res["loss"]), (gold / f"{name}.pt").stat().st_size, "bytes")
    torch.save(metric_cases(ref_loss), gold / "u0_metrics.pt")
    torch.manual_seed(0)
    torch.save(dict(seed=S.INIT_SEED, digests=S.init_digests(RefUNet(), lambda m: ref_init(method=m))), gold / "u0_init.pt")
    for f in sorted(gold.glob("u*.pt")):
        assert f.stat().st_size < 1 << 20, f
        print(f.name, f.stat().st_size)


if __name__ == "__main__":
    main()
