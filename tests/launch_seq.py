"""The library calls an engine issues for one pass, reduced to what decides WHAT runs: the entry-point name of every launch, and
for the two descriptor structs every non-pointer field (pointers: null or not).  tests/test_launch_sequences_gpu.py compares these
sequences with tests/golden/launch_sequences.json; the helper uses nothing but ``hip.LaunchRecorder`` and ctypes, so that

    python tests/launch_seq.py tests/golden/launch_sequences.json        (on an MI355X, from the repository root)

writes the fixture from ANY revision of the package that is first on sys.path (the committed file: the revision before the
prepared-launch API of pmoe_amd/ops.py).

tests/golden/launch_sequences_scalars.json holds the second reduction, ``reduce_scalars``: every ARGUMENT of every call, so that
the row counts, partition counts, ReLU flags and element counts of the launches without a descriptor (the BatchNorm, GAP and
stem-tail passes) are pinned too.  Written the same way, with PYTHONPATH naming a checkout of the other revision (the committed file:
the revision before the engines' BatchNorm hand-offs became named records)."""
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


def reduce_scalars(calls):
    """[(ctypes function, arguments)] of a LaunchRecorder -> [[name, argument ...]], every argument by the entry point's
    ``argtypes``: integers and floats as their values, descriptors as in ``reduce_calls``, everything else -- pointers, pointer
    tables, streams, and the 64-bit dropout seeds, which no case makes reproducible -- as null / non-null (zero / non-zero)"""
    out = []
    for (fn, args), rec in zip(calls, reduce_calls(calls)):
        row = [rec[0]]
        for a, t in zip(args, fn.argtypes):
            if isinstance(getattr(a, "_obj", None), C.Structure):
                row.append(rec[1])
            elif t in (C.c_int32, C.c_int64):
                row.append(int(a))
            else:
                row.append(float(a) if t is C.c_float else bool(a))
        out.append(row)
    return out


def field(rec, name):
    """a descriptor field of a reduced pmoe_conv2d_igemm / pmoe_conv2d_wgrad record"""
    from pmoe_amd import hip
    desc = hip.ConvDesc if rec[0] == "pmoe_conv2d_igemm" else hip.WgradDesc
    return rec[1][[f for f, _ in desc._fields_].index(name)]


def _mixture(fp8, kind="moe", dtype=torch.bfloat16, train=True):
    from oracle import weights as W
    from pmoe_amd.loss import moe_loss
    from pmoe_amd.model.moe import get_model
    from pmoe_amd.utils import stage2_model_cfg
    model = W.fill_state_dict(get_model(stage2_model_cfg(kind, 2, dropout=0.0)), seed=3).to("cuda")
    model.compute_dtype, model.fp8_weights = dtype, fp8
    model.train(train)
    # fp8: layer2 has 4 * 32 * 32 = 4096 pixels per expert (the block-scaled kernel's floor), layer3 / layer4 fewer
    inp = {k: v.cuda() for k, v in W.make_inputs(4 if fp8 else 2, *((128, 128) if fp8 else (64, 64)), seed=5).items()}

    def run():
        with torch.set_grad_enabled(train and not fp8):
            dist, speeds = model(inp["images"], inp["speed"], inp["command"])
            if train and not fp8:
                moe_loss(dist, speeds, inp["control"], inp["target_speed"], [0.7, 0.3]).backward()
        return [t.detach() for t in dist.hip_params] + [speeds.detach()]
    return model, run


def _punet(tmp, batch, side, taped=False, future=2):
    from oracle import weights as W
    from pmoe_amd.utils import build_product
    model = W.fill_state_dict(build_product(Path(tmp), dict(type="punet", n_experts=1, future_frames=future)), seed=3).to("cuda")
    model.compute_dtype = torch.bfloat16
    model.train()
    inp = {k: v.cuda() for k, v in W.make_inputs(batch, side, side, seed=5).items()}

    def run():
        with torch.set_grad_enabled(taped):
            act, sp = model(inp["images"], inp["speed"], inp["command"])
            if taped:                   # (the trainable half: 138-channel stem, ResNet, heads; the PU-Net is frozen)
                (act.square().mean() + sp.square().mean()).backward()
        return [act.detach(), sp.detach()]
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


def _stage1(tmp):
    """PredictiveUnet as tests/test_stage1_gpu.py builds it: ``unet`` frozen, entry block and ``pred_unet`` trained through time"""
    from oracle import weights as W
    from pmoe_amd.loss import AutoregressiveCriterion
    from pmoe_amd.model.blocks import UNet
    from pmoe_amd.model.punet import PredictiveUnet
    Path(tmp).mkdir(parents=True, exist_ok=True)
    torch.save({"unet": UNet().state_dict()}, Path(tmp) / "unet.pth")
    model = PredictiveUnet(past_frames=4, future_frames=3, model_name="unet", model_path=str(Path(tmp) / "unet.pth"))
    model = W.fill_state_dict(model, seed=3).to("cuda")
    model.compute_dtype = torch.bfloat16
    model.train()
    images = W.make_inputs(2, 32, 32, seed=5)["images"].cuda()
    target = W.make_seg_targets(2, 3, 32, 32, 23, seed=7).cuda()

    def run():
        out = model(images)
        AutoregressiveCriterion(3, "tversky")(out, target).backward()
        return [out.detach()]
    return model, run


def engine_cases(tmp):
    """name -> () -> (model, run): the passes of tests/golden/launch_sequences_engines.json -- where the fallbacks behind the
    engines' fused paths run (eval mode, f32, the alpha MLP of ``moe_alt``) and the taped PU-Net classes (the expert's trainable
    half, stage-1 back-propagation through time).  Two predicted frames give the expert a 46-channel stem in 48-wide rows; six
    give the 138 channels that are stored in rows of 192 (``_f6``).  Recorded from the revision before the engines' options were
    reduced to the tested ones and the U-Net primitives moved under a base class of their own."""
    return {"mixture_eval_bf16": lambda: _mixture(False, train=False),
            "mixture_train_f32": lambda: _mixture(False, dtype=torch.float32),
            "moealt_train_bf16": lambda: _mixture(False, kind="moe_alt"),
            "punet_expert_train_taped": lambda: _punet(tmp, 2, 64, taped=True),
            "punet_expert_train_taped_f6": lambda: _punet(tmp, 2, 64, taped=True, future=6),
            "stage1_train_taped": lambda: _stage1(tmp)}


def cases(tmp):
    """name -> () -> (model, run): the engine passes of the fixture, each on a fresh model (so the first-use weight packs are part
    of every sequence).  The PU-Net shapes: the 1x1 direct kernel serves maps of >= 8192 pixels per expert with power-of-two
    sides -- B = 2 at 64 x 64 has them at the top level only (the classifier), B = 2 at 128 x 128 also one level down (the last
    ConvTranspose2d's input) and nowhere below, B = 1 at 64 x 64 nowhere."""
    return {"mixture_train_bf16": lambda: _mixture(False), "mixture_fp8_forward": lambda: _mixture(True),
            "punet_untaped_train_forward": lambda: _punet(tmp, 2, 64), "unet_train_taped": _unet,
            "punet_untaped_train_forward_b2_128": lambda: _punet(tmp, 2, 128),
            "punet_untaped_train_forward_b1_64": lambda: _punet(tmp, 1, 64)}


def scalar_cases(tmp):
    """name -> () -> (model, run): the passes of tests/golden/launch_sequences_scalars.json, taken from the two tables above"""
    both = {**cases(tmp), **engine_cases(tmp)}
    return {name: both[name] for name in ("mixture_train_bf16", "mixture_train_f32", "mixture_eval_bf16",
                                          "punet_untaped_train_forward_b2_128", "punet_expert_train_taped", "stage1_train_taped")}


def record(make, reduce=reduce_calls):
    """-> (model, run, reduced sequence of one run, its outputs)"""
    from pmoe_amd import hip
    hip.load()                          # (the call that loads the library would not be recorded)
    model, run = make()
    with hip.LaunchRecorder() as rec:
        outs = run()
    torch.cuda.synchronize()
    return model, run, reduce(rec.calls), [o.clone() for o in outs]


if __name__ == "__main__":
    import tempfile
    which, reduce = {"launch_sequences_engines.json": (engine_cases, reduce_calls),
                     "launch_sequences_scalars.json": (scalar_cases, reduce_scalars)}.get(Path(sys.argv[1]).name, (cases, reduce_calls))
    with tempfile.TemporaryDirectory() as tmp:
        seqs = {name: record(make, reduce)[2] for name, make in which(tmp).items()}
    body = ",\n".join(json.dumps(k) + ":[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]" for k, v in seqs.items())
    Path(sys.argv[1]).write_text("{" + body + "}\n")
    import pmoe_amd
    print("recorded from", Path(pmoe_amd.__file__).parent, {k: len(v) for k, v in seqs.items()})
