"""The files the progressive tests share (tests/test_pjpeg_cpu.py,
tests/test_gpu_pjpeg.py): Pillow's progressive files with their baseline twins,
the scan scripts Pillow never writes (tests/progressive_ref.py's writer), and
hostile files whose defect holds by construction.  Everything is seeded and
cached: a file and its reference decode are computed once per process."""
import functools
import io

import numpy as np
from PIL import Image

import interleaved_ref as il
import progressive_ref as pr

# (H, W, Pillow subsampling or 'L', restart_marker_rows)
PILLOW_SIZES = [(1, 1, 0, 0), (9, 9, 2, 0), (17, 33, 0, 0), (37, 53, 1, 0), (40, 56, 2, 0), (200, 264, 2, 0),
                (264, 200, 0, 0), (24, 40, 'L', 0), (100, 75, 2, 1)]
QUALITIES = (30, 75, 95)
PILLOW_IDS = [f'{h}x{w}-{ss}{"-rst" if r else ""}-q{q}' for h, w, ss, r in PILLOW_SIZES for q in QUALITIES]
PILLOW_PARAMS = [(h, w, ss, r, q) for h, w, ss, r in PILLOW_SIZES for q in QUALITIES]


@functools.lru_cache(maxsize=None)
def image(H, W, gray=False):
    """A picture with structure and texture (seeded): a gradient, a few edges and noise."""
    rng = np.random.default_rng(1000 * H + W + (7 if gray else 0))
    y, x = np.mgrid[0:H, 0:W]
    base = 96 + 70 * np.sin(x / 9.0) * np.cos(y / 13.0) + 40 * ((x // 16 + y // 12) % 2)
    ch = [base + rng.normal(0, 12, (H, W)) + 25 * k for k in range(1 if gray else 3)]
    a = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return a[:, :, 0] if gray else a


def save(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, 'JPEG', **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pillow_pair(H, W, ss, rst, q):
    """-> (array, progressive file, baseline twin, Pillow's keyword arguments without `progressive`)."""
    arr = image(H, W, ss == 'L')
    kw = {'quality': q}
    if ss != 'L':
        kw['subsampling'] = ss
    if rst:
        kw['restart_marker_rows'] = rst
    return arr, save(arr, progressive=True, **kw), save(arr, **kw), tuple(sorted(kw.items()))


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


# --- scripted files ---------------------------------------------------------

QT = {0: np.full((8, 8), 2.0), 1: np.full((8, 8), 3.0)}
SCRIPT_GEOS = [(24, 40, '4:2:0'), (17, 33, '4:4:4')]


@functools.lru_cache(maxsize=None)
def padded(H, W, mode, amp=40):
    return il.random_padded(np.random.default_rng(H * 131 + W + amp), H, W, mode, amp=amp)


def _script_variants(mode):
    """{name: (script, write keyword arguments, amplitude)}"""
    v = {name: (s, {}, 40) for name, s in pr.scripts(mode).items()}
    ps = pr.pillow_script(mode)
    v['ids_2_3'] = (ps, {'table_ids': {0: (2, 2), 1: (3, 3), 2: (3, 3)}}, 40)
    v['shared_tables'] = (ps, {'shared_tables': True}, 40)
    v['ri1'] = (ps, {'ri': 1}, 40)
    v['ri5'] = (ps, {'ri': 5}, 40)
    v['full_amplitude'] = (ps, {}, 1023)
    return v


SCRIPT_PARAMS = [(H, W, mode, name) for H, W, mode in SCRIPT_GEOS for name in _script_variants(mode)]
SCRIPT_IDS = [f'{h}x{w}-{m}-{n}' for h, w, m, n in SCRIPT_PARAMS]


@functools.lru_cache(maxsize=None)
def script_file(H, W, mode, name):
    """-> (file, the padded coefficients it was written from, complete)."""
    s, kw, amp = _script_variants(mode)[name]
    p = padded(H, W, mode, amp)
    return pr.write(p, H, W, mode, QT, s, **kw), p, name != 'stops_at_al1'


@functools.lru_cache(maxsize=None)
def eobrun_file():
    """1456 x 1456 gray, 33,124 blocks: every AC coefficient zero except one in the last block, so
    the AC scan is EOBRUN 32767, a second run of the 356 blocks left, and one coefficient.
    -> (file, planar coefficients)."""
    H = W = 1456
    rng = np.random.default_rng(1456)
    g = np.zeros((182, 182, 64), np.int64)
    g[:, :, 0] = rng.integers(-60, 61, (182, 182))
    g[-1, -1, 9] = -5
    f = pr.write([g], H, W, 'gray', {0: np.full((8, 8), 4.0)}, pr.scripts('gray')['full_spectrum'])
    return f, g.reshape(-1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def reference(data):
    """progressive_ref.decode(data)['planar'], once per file."""
    return pr.decode(data)['planar']


# --- hostile files ----------------------------------------------------------

def _scan_ranges(data):
    """[(first byte, end) of each scan's entropy-coded segment], by a marker walk."""
    out, p = [], 2
    while data[p + 1] != 0xD9:
        ln = int.from_bytes(data[p + 2:p + 4], 'big')
        m = data[p + 1]
        p += 2 + ln
        if m == 0xDA:
            e = p
            while not (data[e] == 0xFF and data[e + 1] != 0x00 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            out.append((p, e))
            p = e
    return out


@functools.lru_cache(maxsize=None)
def hostile_files():
    """{name: file}.  Each parses, and each holds a defect of its scan data by construction:
      ones_in_scan_K   the first 16 bits of scan K are ones: no code of a table whose all-ones
                       code is reserved (K.2) -- scans that open with a Huffman symbol
      truncated_final  the second half of the last scan's bytes is gone: a prefix of a valid
                       stream decodes to a prefix of its blocks, then the data end
      run_past_se      band 1..5: the first symbol of the scan is run 15 / size 1
      eobrun_too_long  an AC scan opens with EOB14 and fourteen one-bits: a run of 32767 blocks
                       in a file of fewer
      missing_rst      DRI 1 with one RSTm taken out of a scan
      wrong_rst        DRI 1 with one RSTm carrying the wrong number"""
    H, W, mode = 24, 40, '4:2:0'
    p, ps = padded(H, W, mode), pr.pillow_script(mode)
    good = pr.write(p, H, W, mode, QT, ps)
    out = {}
    rng = _scan_ranges(good)
    for k in (0, 1, 5, 9):
        a, e = rng[k]
        assert e - a >= 4
        out[f'ones_in_scan_{k}'] = good[:a] + b'\xff\x00\xff\x00' + good[a + 4:]
    a, e = rng[-1]
    out['truncated_final'] = good[:a + (e - a) // 2] + good[e:]

    def first_symbol(scan, sym, bits=None):
        def t(i, keys, tk):
            if i != scan:
                return tk
            j = next(n for n, x in enumerate(tk) if x[0] == 's')
            ins = [('s', tk[j][1], sym)] + ([('b',) + bits] if bits else [])
            return tk[:j] + ins + tk[j:]
        return t
    out['run_past_se'] = pr.write(p, H, W, mode, QT, ps, tamper=first_symbol(1, 0xF1, (1, 1)))
    out['eobrun_too_long'] = pr.write(p, H, W, mode, QT, ps, tamper=first_symbol(4, 0xE0, (0x3FFF, 14)))

    def rst(scan, drop):
        def t(i, keys, tk):
            if i != scan:
                return tk
            j = [n for n, x in enumerate(tk) if x[0] == 'r'][2]
            return tk[:j] + ([] if drop else [('r', (tk[j][1] + 3) & 7)]) + tk[j + 1:]
        return t
    out['missing_rst'] = pr.write(p, H, W, mode, QT, ps, ri=1, tamper=rst(5, True))
    out['wrong_rst'] = pr.write(p, H, W, mode, QT, ps, ri=1, tamper=rst(0, False))
    return out
