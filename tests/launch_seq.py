"""The library calls an engine issues for one pass, reduced to what decides WHAT runs: the entry-point name of every launch, and
for the two descriptor structs every non-pointer field (pointers: null or not).  tests/test_launch_sequences_gpu.py compares these
sequences with tests/golden/launch_sequences.json; the helper uses nothing but ``hip.LaunchRecorder`` and ctypes, so that

    python tests/launch_seq.py tests/golden/launch_sequences.json        (on an MI355X, from the repository root)

writes the fixture from ANY revision of the package that is first on sys.path (the committed file: the revision before the
prepared-launch API of pmoe_amd/ops.py)."""
import ctypes as C
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.append(str(ROOT))          # (after PYTHONPATH: another revision of the package named there wins)


def reduce_calls(calls):
    """[(ctypes function, arguments)] of a LaunchRecorder -> [[name, descriptor fields in struct order ...]]"""
    out = []
    for fn, args in calls:
        rec = [fn.__name__]
        for a in args:
            d = getattr(a, "_obj", None)
            if isinstance(d, C.Structure):
                # (part_ws_floats: the capacity of the process-wide K-split scratch, which grows with whatever ran before -- it
                #  goes with its pointer)
                rec.append([bool(getattr(d, f)) if t is C.c_void_p or f == "part_ws_floats" else getattr(d, f) for f, t in d._fields_])
        out.append(rec)
    return out


def field(rec, name):
    """a descriptor field of a reduced pmoe_conv2d_igemm / pmoe_conv2d_wgrad record"""
    from pmoe_amd import hip
    desc = hip.ConvDesc if rec[0] == "pmoe_conv2d_igemm" else hip.WgradDesc
    return rec[1][[f for f, _ in desc._fields_].index(name)]


def _mixture(fp8):
    from oracle import weights as W
    from pmoe_amd.loss import moe_loss
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    model = W.fill_state_dict(get_model(stage2_model_cfg("moe", 2, dropout=0.0)), seed=3).to("cuda")
    model.compute_dtype, model.fp8_weights = torch.bfloat16, fp8
    model.train()
    # fp8: layer2 has 4 * 32 * 32 = 4096 pixels per expert (the block-scaled kernel's floor), layer3 / layer4 fewer
    inp = {k: v.cuda() for k, v in W.make_inputs(4 if fp8 else 2, *((128, 128) if fp8 else (64, 64)), seed=5).items()}

    def run():
        with torch.set_grad_enabled(not fp8):
            dist, speeds = model(inp["images"], inp["speed"], inp["command"])
            if not fp8:
                moe_loss(dist, speeds, inp["control"], inp["target_speed"], [0.7, 0.3]).backward()
        return [t.detach() for t in dist.hip_params] + [speeds.detach()]
    return model, run


def _punet(tmp, batch, side):
    from oracle import weights as W
    from pmoe_amd.utils import build_product
    model = W.fill_state_dict(build_product(Path(tmp), dict(type="punet", n_experts=1, future_frames=2)), seed=3).to("cuda")
    model.compute_dtype = torch.bfloat16
    model.train()
    inp = {k: v.cuda() for k, v in W.make_inputs(batch, side, side, seed=5).items()}

    def run():
        with torch.no_grad():
            act, sp = model(inp["images"], inp["speed"], inp["command"])
        return [act, sp]
    return model, run


def _unet():
    from oracle import weights as W
    from pmoe_amd.model.blocks import UNet
    model = W.fill_state_dict(UNet(), seed=3).to("cuda")
    model.compute_dtype = torch.bfloat16
    model.train()
    img = W.make_inputs(2, 64, 64, seed=5)["images"][:, 0].contiguous().cuda()

    def run():
        model(img).float().square().mean().backward()
        return []
    return model, run


def cases(tmp):
    """name -> () -> (model, run): the engine passes of the fixture, each on a fresh model (so the first-use weight packs are part
    of every sequence).  The PU-Net shapes: the 1x1 direct kernel serves maps of >= 8192 pixels per expert with power-of-two
    sides -- B = 2 at 64 x 64 has them at the top level only (the classifier), B = 2 at 128 x 128 also one level down (the last
    ConvTranspose2d's input) and nowhere below, B = 1 at 64 x 64 nowhere."""
    return {"mixture_train_bf16": lambda: _mixture(False), "mixture_fp8_forward": lambda: _mixture(True),
            "punet_untaped_train_forward": lambda: _punet(tmp, 2, 64), "unet_train_taped": _unet,
            "punet_untaped_train_forward_b2_128": lambda: _punet(tmp, 2, 128),
            "punet_untaped_train_forward_b1_64": lambda: _punet(tmp, 1, 64)}


def record(make):
    """-> (model, run, reduced sequence of one run, its outputs)"""
    from pmoe_amd import hip
    hip.load()                          # (the call that loads the library would not be recorded)
    model, run = make()
    with hip.LaunchRecorder() as rec:
        outs = run()
    torch.cuda.synchronize()
    return model, run, reduce_calls(rec.calls), [o.clone() for o in outs]


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        seqs = {name: record(make)[2] for name, make in cases(tmp).items()}
    body = ",\n".join(json.dumps(k) + ":[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]" for k, v in seqs.items())
    Path(sys.argv[1]).write_text("{" + body + "}\n")
    print({k: len(v) for k, v in seqs.items()})
