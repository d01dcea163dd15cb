"""Inputs the transform tests share (test_transform_cpu.py, test_gpu_transform.py): the sizes at
which each mechanism can go wrong, which operations a mode and size allow, EXIF blocks written
here byte by byte, the orientation image, and the NumPy orientations Pillow's decode is compared
with."""
import functools
import io

import numpy as np
from PIL import Image

import transcode_cases as tc
import transform_ref as xr

OPS = xr.OPS[1:]                                   # the seven operations that change something
NON_TRANSPOSING = ['hflip', 'vflip', 'rot180']
# h, w, mode, operations: whole MCUs take every operation their mode allows; sizes with padding
# on both edges take the transposition alone (it has no size constraint)
SIZES = [(48, 80, '4:2:0', OPS),                   # 3 x 5 MCUs
         (8, 8, '4:4:4', OPS),                     # one block
         (16, 16, '4:2:0', OPS),                   # one MCU
         (32, 48, '4:2:2', NON_TRANSPOSING),
         (37, 53, '4:4:4', ['transpose']), (37, 53, '4:2:0', ['transpose']),
         (17, 33, '4:4:4', ['transpose']), (17, 33, '4:2:0', ['transpose'])]
# 13 x 17 whole MCUs of 6 = 1,326 scan blocks, 21 writer segments; 884 luma blocks = 27.6 tiles
# of 32, so the luma plane ends inside a tile and the chroma planes (221 blocks) span seven each
MEDIUM = (208, 272, '4:2:0', OPS)


def allowed(h, w, mode, trim=False):
    """The operations `transform_ref.output_size` accepts for this file."""
    out = []
    for op in OPS:
        try:
            xr.output_size(h, w, mode, op, trim)
            out.append(op)
        except ValueError:
            pass
    return out


def exif_block(orientation, big=True, count_lie=None, tag_type=3):
    """'Exif\\0\\0' + a TIFF header + IFD0 with Make (inline ASCII) and Orientation.  count_lie: the
    entry count the IFD claims (more than it holds: a truncated IFD)."""
    bo = 'big' if big else 'little'
    u16, u32 = (lambda v: int(v).to_bytes(2, bo)), (lambda v: int(v).to_bytes(4, bo))
    head = (b'MM' if big else b'II') + u16(42) + u32(8)
    entries = u16(0x010F) + u16(2) + u32(4) + b'abc\x00'
    entries += u16(0x0112) + u16(tag_type) + u32(1) + u16(orientation) + b'\x00\x00'
    return b'Exif\x00\x00' + head + u16(2 if count_lie is None else count_lie) + entries + u32(0)


@functools.lru_cache(maxsize=None)
def quadrant_image(h=48, w=80):
    """A bright top-left quadrant on a two-way gradient: every one of the eight orientations of
    it is a different picture."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 100 * x / w, 30 + 120 * y / h, 60 + 50 * (x + y) / (h + w)], -1)
    img[:h // 2, :w // 2] += 90
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def quadrant_file(exif=None, mode='4:4:4', quality=90):
    kw = dict(quality=quality, subsampling=tc.SUBSAMPLING[mode], icc_profile=tc.ICC, comment=tc.COMMENT)
    if exif is not None:
        kw['exif'] = exif
    b = io.BytesIO()
    Image.fromarray(quadrant_image()).save(b, 'JPEG', **kw)
    return b.getvalue()


# the eight orientations of an H x W x 3 array, by NumPy alone
ORIENT = {'none': lambda a: a,
          'hflip': lambda a: a[:, ::-1],
          'vflip': lambda a: a[::-1],
          'transpose': lambda a: a.transpose(1, 0, 2),
          'transverse': lambda a: np.rot90(a, 2).transpose(1, 0, 2),
          'rot90': lambda a: np.rot90(a, -1),      # clockwise
          'rot180': lambda a: np.rot90(a, 2),
          'rot270': lambda a: np.rot90(a, 1)}


def closest_orientation(src_pixels, out_pixels):
    """(name of the closest of the eight orientations with out's shape, its mean absolute
    difference, the smallest difference among the others of that shape)."""
    d = {}
    for name, f in ORIENT.items():
        cand = f(src_pixels)
        if cand.shape == out_pixels.shape:
            d[name] = float(np.mean(np.abs(cand.astype(np.int32) - out_pixels.astype(np.int32))))
    best = min(d, key=d.get)
    return best, d[best], min(v for k, v in d.items() if k != best)


def extreme_coeffs(h, w, mode, seed):
    """Random int16 coefficients on the T.81 grids of h x w, -32768 and 32767 among them, every
    block and every position distinct enough that a wrong block or a wrong entry shows."""
    import interleaved_ref as il
    rng = np.random.default_rng(seed)
    _, grids, _ = il.geometry(h, w, mode)
    n = 64 * sum(r * c for r, c in grids)
    cf = rng.integers(-32768, 32768, n).astype(np.int16)
    cf[rng.integers(0, n, max(4, n // 50))] = -32768
    cf[rng.integers(0, n, max(4, n // 50))] = 32767
    cf[0], cf[-1] = -32768, 32767
    return cf, {'H': h, 'W': w, 'mode': mode, 'grids': grids}
