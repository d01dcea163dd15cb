"""libjpeg's default compressor up to the quantised coefficients, in NumPy (DESIGN.md "libjpeg
encoding"): what jds.codec.host_rgb_forward and k_jpeg_fwd are compared against, itself pinned to
Pillow (tests/test_jpeg_forward_cpu.py: the tables are the file's DQTs, the coefficients are the
file's on its T.81 grids).

    tables(quality) -> (2, 8, 8) int64            jpeg_set_quality(Q, force_baseline): luma, chroma
    forward(image, quality, mode) -> (planar int16, info dict)
        image: HxWx3 uint8 (mode '4:4:4', '4:2:2', '4:2:0') or HxW uint8 (mode 'gray');
        planar: jds.entropy.decode_jpeg's layout; info: 'H', 'W', 'mode', 'grids', 'qtables'
        (3, 8, 8), 'tq' -- what jds.entropy.encode_jpeg takes.

The steps are jccolor's 16-bit fixed-point RGB -> YCbCr, jcsample's h2v1 / h2v2 box downsampling
with its alternating bias (edges: the image replicated to the right and bottom, but the bottom
rows of a vertically subsampled plane are copies of its last DOWNSAMPLED row), the level shift,
jfdctint's ISLOW forward DCT (CONST_BITS 13, PASS1_BITS 2, rows then columns, 8x the true DCT)
and the quantiser's rounded division by 8 q.  Every value fits 32 bits; int64 is used throughout."""
import numpy as np

from libjpeg_ref import F, SUB

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)


def tables(quality):
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA, CHROMA)])


def geometry(H, W, mode):
    """-> [(rows, cols)] * 3 block grids and the chroma plane (ch, cw); gray: one grid, no plane."""
    if mode == 'gray':
        return [(-(-H // 8), -(-W // 8)), (0, 0), (0, 0)], (0, 0)
    hmax, vmax = SUB[mode]
    ch, cw = -(-H // vmax), -(-W // hmax)
    return [(-(-H // 8), -(-W // 8))] + [(-(-ch // 8), -(-cw // 8))] * 2, (ch, cw)


def colour(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def full_plane(p, rows, cols):
    """Sample (r, x) of a grid = the plane's sample at (min(r, h-1), min(x, w-1))."""
    h, w = p.shape
    return p[np.minimum(np.arange(rows), h - 1)][:, np.minimum(np.arange(cols), w - 1)]


def chroma_plane(c, mode, rows, cols):
    """The rows x cols samples of a chroma grid from the converted full-resolution plane c (H x W)."""
    H, W = c.shape
    hmax, vmax = SUB[mode]
    if hmax == 1:
        return full_plane(c, rows, cols)
    x = np.arange(cols)
    x0, x1 = np.minimum(2 * x, W - 1), np.minimum(2 * x + 1, W - 1)
    if vmax == 1:
        rr = np.minimum(np.arange(rows), H - 1)
        return (c[rr][:, x0] + c[rr][:, x1] + (x & 1)) >> 1
    rp = np.minimum(np.arange(rows), -(-H // 2) - 1)           # the chroma row is clamped first
    r0, r1 = np.minimum(2 * rp, H - 1), np.minimum(2 * rp + 1, H - 1)
    return (c[r0][:, x0] + c[r0][:, x1] + c[r1][:, x0] + c[r1][:, x1] + 1 + (x & 1)) >> 2


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first):
    """jfdctint's pass over the first axis of d (8, ...): first=True the row pass (results scaled
    up by PASS1_BITS), else the column pass (the scaling removed)."""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * F['c0_541']
    out[2] = descale(z1 + t13 * F['c0_765'], n)
    out[6] = descale(z1 - t12 * F['c1_847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['c1_175']
    t4, t5, t6, t7 = t4 * F['c0_298'], t5 * F['c2_053'], t6 * F['c3_072'], t7 * F['c1_501']
    z1, z2 = -z1 * F['c0_899'], -z2 * F['c2_562']
    z3, z4 = -z3 * F['c1_961'] + z5, -z4 * F['c0_390'] + z5
    out[7], out[5], out[3], out[1] = (descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n),
                                      descale(t7 + z1 + z4, n))
    return np.stack(out)


def fdct_blocks(b):
    """(n, 8, 8) level-shifted samples -> (n, 8, 8): 8x the DCT, row-major [v][u]."""
    rows = fdct_1d(b.transpose(2, 0, 1), True)                 # over the column index -> (u, n, row)
    return fdct_1d(rows.transpose(2, 1, 0), False).transpose(1, 0, 2)   # over the row index -> (v, n, u)


def quantise(c, q):
    d = 8 * q
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def plane_coeffs(p, q):
    """A plane of whole blocks (8 gr x 8 gc samples in 0..255) -> (gr * gc * 64,) quantised."""
    gr, gc = p.shape[0] // 8, p.shape[1] // 8
    b = (p - 128).reshape(gr, 8, gc, 8).transpose(0, 2, 1, 3).reshape(gr * gc, 8, 8)
    return quantise(fdct_blocks(b), q.reshape(1, 8, 8)).reshape(-1)


def forward(image, quality, mode):
    img = np.asarray(image)
    assert img.dtype == np.uint8 and img.ndim == (2 if mode == 'gray' else 3)
    H, W = img.shape[:2]
    grids, _ = geometry(H, W, mode)
    t = tables(quality)
    qt = np.zeros((3, 8, 8))
    qt[0] = t[0]
    if mode == 'gray':
        planar = plane_coeffs(full_plane(img.astype(np.int64), 8 * grids[0][0], 8 * grids[0][1]), t[0])
        return planar.astype(np.int16), {'H': H, 'W': W, 'mode': mode, 'grids': grids, 'qtables': qt, 'tq': [0, 0, 0]}
    qt[1] = qt[2] = t[1]
    y, cb, cr = colour(img)
    parts = [plane_coeffs(full_plane(y, 8 * grids[0][0], 8 * grids[0][1]), t[0])]
    for c in (cb, cr):
        parts.append(plane_coeffs(chroma_plane(c, mode, 8 * grids[1][0], 8 * grids[1][1]), t[1]))
    return np.concatenate(parts).astype(np.int16), {'H': H, 'W': W, 'mode': mode, 'grids': grids, 'qtables': qt,
                                                    'tq': [0, 1, 1]}
