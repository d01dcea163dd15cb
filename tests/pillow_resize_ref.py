"""The definition of Pillow resizing (DESIGN.md "Pillow resizing") in NumPy: Pillow's 8-bit
Image.resize restated -- ImagingResample's coefficients (built in double, converted to 22-bit
fixed point), its two separable passes with the uint8 rounding between them, the passes it
skips, and Image.resize's own rules (the identity copy, very tall images vertically first).
tests/test_resize_cpu.py holds it against the installed Pillow, which is the yardstick."""
import math

import numpy as np

PB = 22
LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5       # Pillow's filter numbers
NAMES = {LANCZOS: 'lanczos', BILINEAR: 'bilinear', BICUBIC: 'bicubic', BOX: 'box', HAMMING: 'hamming'}


def f_box(x):
    return 1.0 if (x > -0.5 and x <= 0.5) else 0.0


def f_bil(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def f_ham(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def f_bic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def f_lan(x):
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


F = {LANCZOS: (f_lan, 3.0), BILINEAR: (f_bil, 1.0), BICUBIC: (f_bic, 2.0), BOX: (f_box, 0.5), HAMMING: (f_ham, 1.0)}


def coeffs(inSize, in0, in1, outSize, flt):
    """One axis: K[xx, x] the taps of output sample xx, B[xx] = (first input sample, count)."""
    f, sup = F[flt]
    in0 = float(np.float32(in0))
    scale = float(np.float32(in1) - np.float32(in0)) / outSize      # box edges are C floats
    fs = max(scale, 1.0)
    support = sup * fs
    ksize = int(math.ceil(support)) * 2 + 1
    K = np.zeros((outSize, ksize), np.int64)
    B = np.zeros((outSize, 2), np.int64)
    for xx in range(outSize):
        center = in0 + (xx + 0.5) * scale
        ss = 1.0 / fs
        xmin = max(int(center - support + 0.5), 0)                  # int(): C truncation
        xmax = min(int(center + support + 0.5), inSize) - xmin      # a COUNT from here on
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v                                                 # in this order
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            K[xx, x] = int(-0.5 + v * (1 << PB)) if v < 0 else int(0.5 + v * (1 << PB))
        B[xx] = (xmin, xmax)
    return K, B


def clip8(s):
    return np.clip(s >> PB, 0, 255).astype(np.uint8)               # arithmetic shift, then clamp


def resize_c(img, size, flt, box):
    """ImagingResample: horizontal, then vertical."""
    H, W = img.shape[:2]
    ow, oh = size
    needh = ow != W or box[0] != 0 or box[2] != W
    needv = oh != H or box[1] != 0 or box[3] != H
    Kh, Bh = coeffs(W, box[0], box[2], ow, flt)
    Kv, Bv = coeffs(H, box[1], box[3], oh, flt)
    y0 = int(Bv[0, 0])
    y1 = int(Bv[-1, 0] + Bv[-1, 1])
    cur = img.astype(np.int64)
    if needh:
        rows = cur[y0:y1] if needv else cur                         # only the rows the vertical pass reads
        t = np.zeros((rows.shape[0], ow, 3), np.int64)
        for xx in range(ow):
            a, n = Bh[xx]
            t[:, xx] = (1 << (PB - 1)) + np.tensordot(rows[:, a:a + n], Kh[xx, :n], axes=([1], [0]))
        cur = clip8(t).astype(np.int64)                             # the intermediate is uint8
        if needv:
            Bv = Bv.copy()
            Bv[:, 0] -= y0
    if needv:
        t = np.zeros((oh, cur.shape[1], 3), np.int64)
        for yy in range(oh):
            a, n = Bv[yy]
            t[yy] = (1 << (PB - 1)) + np.tensordot(cur[a:a + n], Kv[yy, :n], axes=([0], [0]))
        cur = clip8(t).astype(np.int64)
    return cur.astype(np.uint8)


def resize(img, size, flt, box=None):
    """Image.resize of Pillow 12: size = (width, height), img HxWx3 uint8."""
    H, W = img.shape[:2]
    ow, oh = size
    box = box or (0, 0, W, H)
    if (W, H) == tuple(size) and tuple(box) == (0, 0, W, H):
        return img.copy()
    if H > W * 100 and oh < H:                                      # very tall images: vertically first
        t = resize_c(img, (W, oh), flt, (0, box[1], W, box[3]))
        return resize_c(t, size, flt, (box[0], 0, box[2], oh))
    return resize_c(img, size, flt, box)
