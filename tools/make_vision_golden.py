#!/usr/bin/env python3
"""Write tests/golden/vision.npz: inputs and the outputs of the reference's ``utils/vision.py`` (``decode_mask``,
``draw_on_image``) for them.  Runs on the CPU:

    python tools/make_vision_golden.py <path to the reference's utils/vision.py>

The reference module is imported as it is, behind these shims: stub modules for ``matplotlib`` / ``torchvision`` where they are not
installed (only ``plot_images`` uses them), ``np.float = float`` where numpy no longer has it, and ``ImageFont.truetype`` /
``ImageDraw.text`` replaced by no-ops -- so ``draw_on_image`` returns the normalised frame alone (this project claims no parity
with PIL's font rendering, pmoe_amd/vision.py)."""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).resolve().parents[1] / "tests" / "golden" / "vision.npz"


def load_reference(path):
    for name, subs in (("matplotlib", ("pyplot",)), ("torchvision", ("utils",))):
        try:
            __import__(name)
        except ImportError:
            top = types.ModuleType(name)
            sys.modules[name] = top
            for s in subs:
                sub = types.ModuleType(f"{name}.{s}")
                setattr(top, s, sub)
                sys.modules[f"{name}.{s}"] = sub
    if not hasattr(np, "float"):
        np.float = float
    from PIL import ImageDraw, ImageFont
    ImageFont.truetype = lambda *a, **k: None
    ImageDraw.ImageDraw.text = lambda self, *a, **k: None
    spec = importlib.util.spec_from_file_location("reference_vision", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(12)
    logits = rng.standard_normal((23, 12, 16)).astype(np.float32)
    # planted ties: the maximum twice (the lower index wins), all classes equal, the last two classes equal
    logits[[3, 17], 0, 0] = 9.0
    logits[:, 0, 1] = 0.5
    logits[[21, 22], 5, 7] = 7.25
    logits[[0, 22], 11, 15] = 8.0
    ids = rng.integers(0, 23, (12, 16)).astype(np.int64)
    ids[0, :4] = (22, 23, 255, 0)
    ids[11, 15] = 22
    frames = rng.standard_normal((2, 3, 20, 28)).astype(np.float32)
    frames[1] = frames[1] * 40.0 + 100.0
    meas = dict(control=torch.tensor([0.25, -0.5]), speed=torch.tensor([0.5]), command=torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))
    action = torch.tensor([-0.125, 0.75])
    drawn = np.stack([ref.draw_on_image(torch.from_numpy(f), meas, action, gt) for f, gt in zip(frames, (True, False))])
    assert drawn.dtype == np.uint8 and drawn.shape == (2, 20, 28, 3)
    np.savez_compressed(OUT, logits=logits, logits_rgb=ref.decode_mask(logits), ids=ids, ids_rgb=ref.decode_mask(ids),
                        ids_rgb_nc5=ref.decode_mask(ids, nc=5), frames=frames, frames_u8=drawn)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
