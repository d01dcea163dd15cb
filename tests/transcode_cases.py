"""Inputs the transcode tests share (test_transcode_cpu.py, test_gpu_transcode.py): Pillow
files of every mode with and without metadata, restart files, foreign files with non-zero
padding blocks and other table assignments, the stuffing and K.3 cases, the file that is
decodable but not baseline-codable once its restart intervals are joined."""
import functools
import io

import numpy as np
from PIL import Image

import huff_hostile as hh
import huffopt_ref as hr
import interleaved_ref as ir
from oracle import cpu_ref

SUBSAMPLING = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
MODES = ['4:4:4', '4:2:2', '4:2:0']
Q50 = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50)
QC = np.clip(Q50 * 2 + 3, 1, 255)
EXIF = b'Exif\x00\x00MM\x00*\x00\x00\x00\x08\x00\x00'
ICC = bytes(range(256)) * 3
COMMENT = b'transcode keeps this comment'


@functools.lru_cache(maxsize=None)
def image(h, w, seed=0):
    """Smooth structure plus noise: every size has DC steps, runs, EOBs and a few long codes."""
    rng = np.random.default_rng(1000 * h + w + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0)
    img = base[:, :, None] + rng.normal(0, 25, (h, w, 3)) + np.array([0, 20, -20])
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pillow(h, w, mode, quality=50, optimize=False, meta=False, restart_rows=0, seed=0, noise=False):
    """Pillow's (libjpeg's) file of image(h, w): plain or optimize=True, with EXIF + ICC + COM or
    bare, with restart_marker_rows or without."""
    img = image(h, w, seed)
    if noise:
        img = np.random.default_rng(h * w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    kw = dict(quality=quality, subsampling=SUBSAMPLING[mode], optimize=optimize)
    if meta:
        kw.update(exif=EXIF, icc_profile=ICC, comment=COMMENT)
    if restart_rows:
        kw['restart_marker_rows'] = restart_rows
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', **kw)
    return b.getvalue()


def pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


@functools.lru_cache(maxsize=None)
def foreign(h, w, mode, seed, scan_tables=ir.STD_SCAN_TABLES, tq=(0, 1, 1), ri=0, three_scans=False):
    """interleaved_ref.write (or huff_hostile.write3) over random_padded: non-zero padding blocks
    with distinct DCs, the table ids and quantisation table ids as given."""
    rng = np.random.default_rng(seed)
    padded = ir.random_padded(rng, h, w, mode)
    qt = {i: (Q50, QC, np.clip(QC + 7, 1, 255))[i] for i in sorted(set(tq))}
    if three_scans:
        return hh.write3(padded, h, w, mode, qt, tq=tq, scan_tables=scan_tables, ri=ri)
    return ir.write(padded, h, w, mode, qt, tq=tq, scan_tables=scan_tables, ri=ri)


FOREIGN_CASES = [
    # h, w, mode, seed, scan_tables, tq, ri, three_scans
    (17, 33, '4:2:0', 1, ir.STD_SCAN_TABLES, (0, 1, 1), 0, False),
    (17, 33, '4:2:0', 2, ((1, 1), (0, 0), (0, 1)), (0, 1, 2), 0, False),
    (37, 53, '4:2:2', 3, ((0, 1), (1, 0), (1, 1)), (0, 0, 0), 0, False),
    (37, 53, '4:4:4', 4, ((1, 0), (1, 0), (0, 1)), (1, 0, 0), 0, False),
    (37, 53, '4:2:0', 5, ir.STD_SCAN_TABLES, (0, 1, 1), 2, False),
    (24, 40, '4:2:2', 6, ((1, 1), (0, 0), (0, 0)), (0, 1, 1), 1, False),
    (37, 53, '4:2:0', 7, ((1, 1), (0, 0), (0, 1)), (0, 1, 1), 0, True),
    (17, 33, '4:4:4', 8, ir.STD_SCAN_TABLES, (0, 1, 2), 5, True),
]


def not_codable():
    """A restart file (4:4:4, 16 x 32, two intervals of four MCUs) whose intervals hold luma DCs
    of +1500 and -1500: every interval is codable from prediction 0 (category 11), joined the
    step is -3000 (category 12)."""
    h, w, mode = 16, 32, '4:4:4'
    padded = [np.zeros(s + (64,), np.int64) for s in ir.padded_shapes(h, w, mode)]
    padded[0][0, :, 0] = 1500
    padded[0][1, :, 0] = -1500
    padded[0][:, :, 1] = 3
    return ir.write(padded, h, w, mode, {0: Q50, 1: QC}, ri=4)


def k3_coeffs():
    """(coeffs, info dict): a 104 x 104 4:4:4 frame whose AC luma histogram is Fibonacci-steep, so
    the unconstrained code is 17 bits long and K.3 acts (test_huffopt_cpu's case)."""
    hist = hr.steep_ac_histogram([int(v) for v in hr.fibonacci(17)[:17]], 10)
    blk = hr.blocks_with_ac_histogram(169, hist)
    cf = np.concatenate([blk, np.zeros((2 * 169, 64), np.int16)]).reshape(-1)
    return cf, info_of(104, 104, '4:4:4'), hist


def info_of(h, w, mode, qtables=None, tq=(0, 1, 1)):
    """encode_jpeg's info dict for an h x w frame on its T.81 grids."""
    _, grids, _ = ir.geometry(h, w, mode)
    q = np.stack([Q50, QC, QC]) if qtables is None else np.asarray(qtables)
    return {'H': h, 'W': w, 'mode': mode, 'grids': grids, 'qtables': q, 'tq': list(tq)}


def random_coeffs(h, w, mode, seed):
    rng = np.random.default_rng(seed)
    _, grids, _ = ir.geometry(h, w, mode)
    return ir.crop(ir.random_padded(rng, h, w, mode), grids)
