"""numpy restatement of pmoe_amd.vision's contract (include/pmoe_hip.h: pmoe_decode_mask, pmoe_frame_annotate), written from the
rules: the arg-max, the palette lookup and its division; the f32 normalisation; the strings, their numbers formatted in integers;
the bitmap glyphs, positions, colours and order.  The device result equals it bit for bit."""
import struct

import numpy as np

from pmoe_amd.vision import CARLA_PALETTE, FONT, TEXT_COLS, TEXT_ROWS

PALETTE = CARLA_PALETTE.numpy()
RED, GREEN = (255, 0, 0), (0, 255, 0)


def argmax_first(values):
    """numpy's rule, spelled out: the lowest index wins a tie, a NaN is the maximum and the first NaN wins"""
    best, bi = values[0], 0
    for i, v in enumerate(values[1:], 1):
        if best == best and (v > best or v != v):
            best, bi = v, i
    return bi


def decode_mask_ref(mask, nc=23, palette=PALETTE, dtype=np.float64):
    """mask: f32 [..., C, H, W] logits or integer [..., H, W] ids -> [..., 3, H, W] (float dtypes) or [..., H, W, 3] (uint8)"""
    mask = np.asarray(mask)
    ids = np.argmax(mask, axis=-3) if mask.dtype == np.float32 else mask.astype(np.int64)
    inside = (ids >= 0) & (ids < nc)
    rgb = np.where(inside[..., None], np.asarray(palette, dtype=np.uint8)[np.where(inside, ids, 0)], 0).astype(np.uint8)
    if dtype == np.uint8:
        return rgb
    return np.moveaxis(rgb, -1, -3).astype(dtype) / dtype(255)


def normalise_ref(img):
    """f32 [3, H, W] -> uint8 [H, W, 3]: one f32 rounding per operation, a NaN ignored by the extrema, 0 where the value is not
    in [0, 255] (a constant frame, a NaN pixel)"""
    img = np.asarray(img, dtype=np.float32)
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(img, axis=None, initial=np.float32(np.inf))
        hi = np.fmax.reduce(img, axis=None, initial=np.float32(-np.inf))
        v = ((img - np.float32(lo)) / (-np.float32(lo) + np.float32(hi))) * np.float32(255.0)
        assert v.dtype == np.float32
        ok = (v >= 0) & (v <= 255)
        out = np.where(ok, v, 0).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def fmt3(x):
    """"%.3f" of an f32, in integers"""
    bits = struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]
    ex, mant = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if ex == 0xFF and mant:
        return "nan"
    sign = "-" if bits >> 31 else ""
    if ex == 0xFF:
        return sign + "inf"
    if ex >= 127 + 20:
        return sign + "big"
    m = ((mant | 0x800000) if ex else mant) * 1000
    s = 150 - ex if ex else 149
    q, rem, half = m >> s, m & ((1 << s) - 1), 1 << (s - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return "%s%d.%03d" % (sign, q // 1000, q % 1000)


def _pedal(pedal):
    """-> (throttle string, brake string)"""
    pedal = np.float32(pedal)
    return (fmt3(pedal), "0.000") if pedal > 0 else ("0.000", fmt3(-pedal))


def strings_ref(action, command, speed=None, control_gt=None, gt=False):
    """-> the TEXT_ROWS strings of one frame in drawing order (empty: not drawn)"""
    throttle, brake = _pedal(action[1])
    rows = ["Steer: " + fmt3(action[0]), "Throttle: " + throttle, "Brake: " + brake,
            "Command: %d" % argmax_first([np.float32(c) for c in command])]
    if gt:
        throttle, brake = _pedal(control_gt[1])
        rows += ["Speed: " + fmt3(np.asarray(speed).reshape(-1)[0]), "Steer: " + fmt3(control_gt[0]), "Throttle: " + throttle,
                 "Brake: " + brake]
    else:
        rows += [""] * 4
    assert len(rows) == TEXT_ROWS
    return rows


def text_codes(rows):
    """-> uint8 [TEXT_ROWS, TEXT_COLS], space padded (what the kernel's text_out holds)"""
    return np.array([[ord(ch) for ch in s[:TEXT_COLS].ljust(TEXT_COLS)] for s in rows], dtype=np.uint8)


def positions(w):
    w2 = w // 2
    return [((5, 30), RED), ((5, 50), RED), ((5, 70), RED), ((w2, 10), GREEN),
            ((5, 10), GREEN), ((w2, 30), GREEN), ((w2, 50), GREEN), ((w2, 70), GREEN)]


def draw_text(out, rows):
    """the strings onto uint8 [H, W, 3] in place, in order, clipped"""
    h, w, _ = out.shape
    for s, ((x0, y0), colour) in zip(rows, positions(w)):
        for i, ch in enumerate(s[:TEXT_COLS]):
            for dy, mask in enumerate(FONT[ch]):
                for dx in range(5):
                    x, y = x0 + 6 * i + dx, y0 + dy
                    if (mask >> (4 - dx)) & 1 and 0 <= x < w and 0 <= y < h:
                        out[y, x] = colour
    return out


def text_region(h, w):
    """bool [H, W]: the pixels some string's cell box can cover"""
    m = np.zeros((h, w), dtype=bool)
    for (x0, y0), _ in positions(w):
        m[y0:y0 + 7, x0:x0 + 6 * TEXT_COLS] = True
    return m


def draw_ref(img, action, command, speed=None, control_gt=None, gt=False):
    """one frame: f32 [3, H, W] -> uint8 [H, W, 3]"""
    return draw_text(normalise_ref(img), strings_ref(action, command, speed, control_gt, gt))
