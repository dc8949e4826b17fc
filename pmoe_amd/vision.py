"""Vision utilities on the device: the reference's ``utils/vision.py`` (``decode_mask`` for the trainers' image logs,
``draw_on_image`` for ``train_2.py`` and the agent's ``run_step``) without a trip to the host, and :class:`FrameLog`, the agent's
``self.vizs`` list as a device ring.

What is the reference's: ``decode_mask``'s arg-max, palette and ``u8 / 255.0`` in double (bit for bit); ``draw_on_image``'s
normalisation ``(((img - min) / (-min + max)) * 255).astype(uint8)`` in f32 (bit for bit), its strings, their numbers, positions,
colours and order.

What is NOT claimed: parity with PIL's TrueType rendering of ``FUTURAM.ttf``.  PIL and the font file are not dependencies of this
project and no glyph here was compared against them.  The text is drawn with the hard-edged 5 x 7 bitmap font ``FONT`` below (a
6-pixel advance, the top-left corner at the string's position, no anti-aliasing), and ``%.3f`` is computed on the device in
integers; the contract is stated in ``include/pmoe_hip.h`` (``pmoe_frame_annotate``) and restated in numpy by
``tests/vision_ref.py``, which the device result equals bit for bit.  Where the reference is undefined -- a constant frame, a NaN
pixel -- the pixel is 0.

Every input and output is a device tensor; there is no CPU path.  Only ``FrameLog.frames()`` synchronises.
"""
import numpy as np
import torch

from .hip import check, load, ptr, stream_ptr

TEXT_ROWS, TEXT_COLS = 8, 24                    # PMOE_TEXT_ROWS, PMOE_TEXT_COLS
MAX_FRAMES = 65535                              # frames per launch
_KIND = {torch.float32: 0, torch.int64: 1, torch.uint8: 2}      # PMOE_MASK_*
_OUT = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}     # PMOE_VIS_*

# CARLA's documented semantic-segmentation colours (carla.readthedocs.io, ref_sensors: semantic segmentation camera), tags 0..22
CARLA_PALETTE = torch.tensor([
    (0, 0, 0),            # 0 Unlabeled
    (70, 70, 70),         # 1 Building
    (100, 40, 40),        # 2 Fence
    (55, 90, 80),         # 3 Other
    (220, 20, 60),        # 4 Pedestrian
    (153, 153, 153),      # 5 Pole
    (157, 234, 50),       # 6 RoadLine
    (128, 64, 128),       # 7 Road
    (244, 35, 232),       # 8 SideWalk
    (107, 142, 35),       # 9 Vegetation
    (0, 0, 142),          # 10 Vehicles
    (102, 102, 156),      # 11 Wall
    (220, 220, 0),        # 12 TrafficSign
    (70, 130, 180),       # 13 Sky
    (81, 0, 81),          # 14 Ground
    (150, 100, 100),      # 15 Bridge
    (230, 150, 140),      # 16 RailTrack
    (180, 165, 180),      # 17 GuardRail
    (250, 170, 30),       # 18 TrafficLight
    (110, 190, 160),      # 19 Static
    (170, 120, 50),       # 20 Dynamic
    (45, 60, 150),        # 21 Water
    (145, 170, 100),      # 22 Terrain
], dtype=torch.uint8)

# The bitmap font, for the characters the strings can contain: seven rows of five columns per glyph, top row first.
_GLYPHS = {
    " ": "..... ..... ..... ..... ..... ..... .....",
    "-": "..... ..... ..... ##### ..... ..... .....",
    ".": "..... ..... ..... ..... ..... .##.. .##..",
    ":": "..... .##.. .##.. ..... .##.. .##.. .....",
    "0": ".###. #...# #..## #.#.# ##..# #...# .###.",
    "1": "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    "2": ".###. #...# ....# ...#. ..#.. .#... #####",
    "3": "##### ...#. ..#.. ...#. ....# #...# .###.",
    "4": "...#. ..##. .#.#. #..#. ##### ...#. ...#.",
    "5": "##### #.... ####. ....# ....# #...# .###.",
    "6": "..##. .#... #.... ####. #...# #...# .###.",
    "7": "##### ....# ...#. ..#.. .#... .#... .#...",
    "8": ".###. #...# #...# .###. #...# #...# .###.",
    "9": ".###. #...# #...# .#### ....# ...#. .##..",
    "B": "####. #...# #...# ####. #...# #...# ####.",
    "C": ".###. #...# #.... #.... #.... #...# .###.",
    "S": ".#### #.... #.... .###. ....# ....# ####.",
    "T": "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    "a": "..... ..... .###. ....# .#### #...# .####",
    "b": "#.... #.... #.##. ##..# #...# #...# ####.",
    "d": "....# ....# .##.# #..## #...# #...# .####",
    "e": "..... ..... .###. #...# ##### #.... .###.",
    "f": "..##. .#..# .#... ###.. .#... .#... .#...",
    "g": "..... .#### #...# #...# .#### ....# .###.",
    "h": "#.... #.... #.##. ##..# #...# #...# #...#",
    "i": "..#.. ..... .##.. ..#.. ..#.. ..#.. .###.",
    "k": "#.... #.... #..#. #.#.. ##... #.#.. #..#.",
    "l": ".##.. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",
    "m": "..... ..... ##.#. #.#.# #.#.# #...# #...#",
    "n": "..... ..... #.##. ##..# #...# #...# #...#",
    "o": "..... ..... .###. #...# #...# #...# .###.",
    "p": "..... ####. #...# #...# ####. #.... #....",
    "r": "..... ..... #.##. ##..# #.... #.... #....",
    "t": ".#... .#... ###.. .#... .#... .#..# ..##.",
}
# char -> 7 row masks, bit 4 = the leftmost column: the one definition of the font (the kernel takes it as a [128][7] table)
FONT = {ch: tuple(int(row.replace("#", "1").replace(".", "0"), 2) for row in art.split()) for ch, art in _GLYPHS.items()}

_tables = {}            # (what, device) -> device tensor


def _device_table(what, device):
    key = (what, device)
    if key not in _tables:
        if what == "font":
            host = torch.zeros(128, 7, dtype=torch.uint8)
            for ch, masks in FONT.items():
                host[ord(ch)] = torch.tensor(masks, dtype=torch.uint8)
        else:
            host = CARLA_PALETTE
        _tables[key] = host.to(device)
    return _tables[key]


def _on_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the MI355X (cuda) device, got {t.device}; pmoe_amd has no CPU path")
    return t


def decode_mask(mask, nc=23, palette=CARLA_PALETTE, dtype=torch.float64):
    """``utils/vision.py:26-85`` on the device, batched.  ``mask``: f32 logits ``[..., C, H, W]`` (the class is numpy's arg-max
    over C: the lowest index wins a tie, a NaN is the maximum and the first NaN wins) or class ids ``[..., H, W]`` (int64 or
    uint8).  An id outside ``[0, nc)`` is black.  ``palette``: uint8 ``[>= nc, 3]``; ``CARLA_PALETTE`` is kept on the device, any
    other one is a device tensor.  -> ``dtype=torch.float64``: ``[..., 3, H, W]`` = ``u8 / 255.0`` divided in double (the
    reference's array, bit for bit); ``torch.float32``: the same layout, one f32 division; ``torch.uint8``: ``[..., H, W, 3]``."""
    _on_device(mask, "decode_mask: mask")
    if mask.dtype not in _KIND:
        raise ValueError(f"decode_mask: f32 logits or int64 / uint8 class ids, got {mask.dtype}")
    if dtype not in _OUT:
        raise ValueError(f"decode_mask: dtype is torch.float64, torch.float32 or torch.uint8, got {dtype}")
    logits = mask.dtype == torch.float32
    if mask.dim() < (3 if logits else 2):
        raise ValueError(f"decode_mask: {'logits [..., C, H, W]' if logits else 'class ids [..., H, W]'}, got {tuple(mask.shape)}")
    lead = tuple(mask.shape[:-3] if logits else mask.shape[:-2])
    c, (h, w) = (mask.shape[-3] if logits else 0), mask.shape[-2:]
    n = int(np.prod(lead, dtype=np.int64))
    nc = int(nc)
    if nc < 1 or n < 1 or h < 1 or w < 1 or (logits and c < 1):
        raise ValueError(f"decode_mask: nc and every extent must be positive, got nc = {nc} and {tuple(mask.shape)}")
    if palette is CARLA_PALETTE:
        palette = _device_table("palette", mask.device)
    if palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < nc or _on_device(palette, "decode_mask: palette").device != mask.device:
        raise ValueError(f"decode_mask: palette must be uint8 [>= {nc}, 3] on {mask.device}, got {tuple(palette.shape)} on {palette.device}")
    out = torch.empty((n, h, w, 3) if dtype == torch.uint8 else (n, 3, h, w), dtype=dtype, device=mask.device)
    src = mask.reshape((n, c, h, w) if logits else (n, h, w))
    pal = ptr(palette, "decode_mask: palette", torch.uint8)
    with torch.cuda.device(mask.device):
        for b0 in range(0, n, MAX_FRAMES):
            nb = min(MAX_FRAMES, n - b0)
            check(load().pmoe_decode_mask(ptr(src[b0:b0 + nb], "decode_mask: mask"), _KIND[mask.dtype], ptr(out[b0:b0 + nb]),
                                          _OUT[dtype], pal, nc, nb, c, h, w, stream_ptr()), "pmoe_decode_mask")
    return out.reshape(lead + tuple(out.shape[1:]))


def _rows(t, b, n, name):
    """f32 device tensor with b * n values -> [b, n] (n None: any row length)"""
    _on_device(t, name)
    if t.dtype != torch.float32 or t.numel() % b or (n is not None and t.numel() != b * n) or t.numel() == 0:
        raise ValueError(f"{name}: expected f32 with {b} row(s)" + (f" of {n}" if n else "") + f", got {t.dtype} {tuple(t.shape)}")
    return t.reshape(b, -1)


def annotate(frames, out, action, command, speed=None, control_gt=None, gt=False, slot=0, text_out=None):
    """One ``pmoe_frame_annotate`` launch on the current stream: ``frames`` f32 ``[B,3,h,w]`` (each frame dense; the batch stride
    is free, so a slot of a frame ring is read in place) are normalised, annotated and written as uint8 into slots ``slot,
    slot + 1, ...`` (wrapping) of ``out [capacity,h,w,3]``.  ``action [B,2]``, ``command [B,n]``; with ``gt`` also ``speed [B]``
    and ``control_gt [B,2]``.  ``text_out``: uint8 ``[B, TEXT_ROWS, TEXT_COLS]`` receives the strings' char codes."""
    _on_device(frames, "annotate: frames")
    _on_device(out, "annotate: out")
    if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3 or 0 in frames.shape:
        raise ValueError(f"annotate: frames must be f32 [B,3,h,w], got {frames.dtype} {tuple(frames.shape)}")
    b, _, h, w = frames.shape
    if b > 1 and frames.stride(0) < 3 * h * w:
        raise ValueError("annotate: the frames overlap")
    if not frames[0].is_contiguous():
        raise ValueError("annotate: each frame must be contiguous")
    cap = out.shape[0] if out.dim() == 4 else 0
    if tuple(out.shape) != (cap, h, w, 3) or b > min(cap, MAX_FRAMES) or not 0 <= slot < cap:
        raise ValueError(f"annotate: {b} frame(s) from slot {slot} of out [capacity >= {b}, {h}, {w}, 3], got {tuple(out.shape)}")
    action, command = _rows(action, b, 2, "annotate: action"), _rows(command, b, None, "annotate: command")
    if gt:
        if speed is None or control_gt is None:
            raise ValueError("annotate: gt needs the speed and the ground-truth control")
        speed, control_gt = _rows(speed, b, 1, "annotate: speed"), _rows(control_gt, b, 2, "annotate: control")
    else:
        speed = control_gt = None
    if text_out is not None and tuple(text_out.shape) != (b, TEXT_ROWS, TEXT_COLS):
        raise ValueError(f"annotate: text_out must be uint8 [{b}, {TEXT_ROWS}, {TEXT_COLS}], got {tuple(text_out.shape)}")
    for t in (out, action, command, speed, control_gt, text_out):
        if t is not None and t.device != frames.device:
            raise ValueError(f"annotate: the frames are on {frames.device}, another argument on {t.device}")
    with torch.cuda.device(frames.device):
        rc = load().pmoe_frame_annotate(frames.data_ptr(), frames.stride(0) if b > 1 else 3 * h * w,
                                        ptr(out, "annotate: out", torch.uint8), b, h, w, slot, cap, ptr(action, "annotate: action"),
                                        ptr(speed, "annotate: speed"), ptr(command, "annotate: command"), command.shape[1],
                                        ptr(control_gt, "annotate: control"), int(bool(gt)),
                                        ptr(_device_table("font", frames.device)), ptr(text_out, "annotate: text_out", torch.uint8),
                                        stream_ptr())
    check(rc, "pmoe_frame_annotate")
    return out


def draw_on_image(img, measurements, action, gt=True):
    """``utils/vision.py:88-152`` on the device: ``img`` f32 ``[3,H,W]`` or ``[B,3,H,W]``, ``measurements`` the reference's dict
    (``control [.,2]``, ``speed [.]`` or ``[.,1]``, ``command [.,n]``; with ``gt=False`` only ``command`` is read and the others
    may be absent), ``action [.,2]`` -> uint8 ``[H,W,3]`` or ``[B,H,W,3]``.  The frame and the strings are the reference's, the
    glyphs are ``FONT``'s (see the module's head)."""
    _on_device(img, "draw_on_image: img")
    if img.dim() not in (3, 4):
        raise ValueError(f"draw_on_image: img must be [3,H,W] or [B,3,H,W], got {tuple(img.shape)}")
    frames = img if img.dim() == 4 else img.unsqueeze(0)
    if frames.dim() == 4 and frames.shape[0] and not frames[0].is_contiguous():
        frames = frames.contiguous()
    if frames.dtype != torch.float32 or frames.shape[1] != 3 or 0 in frames.shape:
        raise ValueError(f"draw_on_image: img must be f32 [3,H,W] or [B,3,H,W], got {img.dtype} {tuple(img.shape)}")
    b, _, h, w = frames.shape
    out = torch.empty(b, h, w, 3, dtype=torch.uint8, device=img.device)
    annotate(frames, out, action, measurements["command"], measurements["speed"] if gt else None,
             measurements["control"] if gt else None, gt=gt)
    return out if img.dim() == 4 else out[0]


class FrameLog:
    """The agent's video log (``image_agent.py``: ``self.vizs.append(draw_on_image(...))``, flushed every 1000 frames) as a device
    ring ``uint8 [capacity, h, w, 3]`` -- 150 MB at the reference's 1000 frames of 224 x 224.  ``push`` is one launch on the
    current stream and never synchronises; when the ring is full the oldest frames are overwritten and counted in ``dropped``.
    ``frames()`` brings the log to the host, oldest first, and is the only call that synchronises."""

    def __init__(self, capacity=1000, size=(224, 224), device="cuda"):
        self.capacity, self.size = int(capacity), (int(size[0]), int(size[1]))
        if self.capacity < 1 or min(self.size) < 1:
            raise ValueError("FrameLog: capacity and size must be positive")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"FrameLog: the ring lives on the MI355X (cuda) device, got {device}; pmoe_amd has no CPU path")
        load()
        self.ring = torch.zeros(self.capacity, *self.size, 3, dtype=torch.uint8, device=device)
        self._host = None
        self.clear()

    @property
    def device(self):
        return self.ring.device

    def clear(self):
        self._next = self._count = self.dropped = 0

    def __len__(self):
        return self._count

    def push(self, frames, action, speed, command, control_gt=None):
        """``frames`` f32 ``[B,3,h,w]`` annotated into the next B slots (``B <= capacity``): the predicted ``action [B,2]`` and the
        ``command [B,n]`` always, the ``speed [B]`` and the ground truth ``control_gt [B,2]`` when the latter is given
        (``draw_on_image``'s ``gt``)."""
        gt = control_gt is not None
        annotate(frames, self.ring, action, command, speed if gt else None, control_gt, gt=gt, slot=self._next)
        b = frames.shape[0]
        self._next = (self._next + b) % self.capacity
        self.dropped += max(0, self._count + b - self.capacity)
        self._count = min(self.capacity, self._count + b)

    def frames(self):
        """-> numpy uint8 ``[len(log), h, w, 3]``, oldest first: at most two device-to-host copies into pinned memory"""
        n = self._count
        if self._host is None:
            self._host = torch.empty(self.ring.shape, dtype=torch.uint8, pin_memory=True)
        first = (self._next - n) % self.capacity
        head = min(n, self.capacity - first)
        with torch.cuda.device(self.ring.device):
            if head:
                self._host[:head].copy_(self.ring[first:first + head], non_blocking=True)
            if n > head:
                self._host[head:n].copy_(self.ring[:n - head], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return self._host[:n].numpy().copy()
