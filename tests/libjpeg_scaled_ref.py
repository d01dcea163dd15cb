"""libjpeg's reduced-size decode (scale 1/2, 1/4, 1/8) of decoded baseline coefficients in NumPy
(DESIGN.md "Scaled libjpeg rendering"): what render='libjpeg' with scale_denom is compared against,
itself pinned to Pillow's Image.draft byte for byte (tests/test_jpeg_scale_cpu.py).

    render_scaled(planar, H, W, mode, qtables, grids, denom) -> ceil(H/denom) x ceil(W/denom) x 3 uint8
        libjpeg_ref.render_coeffs' arguments and the denominator 1, 2, 4 or 8 (1: render_coeffs).

With m = 8 / denom (libjpeg's min_DCT_scaled_size): luma blocks through jidctred's m-point inverse;
chroma through the s-point one, s = m doubled while s < 8 and (Hmax m, Vmax m) are multiples of
2 s; every plane cropped to ceil(side * size / (8 * sampling factor)); the h2v1 upsampling that
4:2:2 keeps is fancy when m > 1 and the cropped plane is more than two samples wide, replication
otherwise; jdcolor's conversion.  Values are taken modulo 2^32 as in libjpeg_ref."""
import numpy as np

from libjpeg_ref import SUB, colour, descale, idct_blocks, upsample_h2v1, wrap32


def chroma_size(m, hmax, vmax):
    s = m
    while s < 8 and (hmax * m) % (2 * s) == 0 and (vmax * m) % (2 * s) == 0:
        s *= 2
    return s


def _idct4(i, n):
    i = [wrap32(v) for v in i]
    t0 = i[0] << 14
    t2 = 15137 * i[2] - 6270 * i[6]
    t10, t12 = t0 + t2, t0 - t2
    a = -1730 * i[7] + 11893 * i[5] - 17799 * i[3] + 8697 * i[1]
    b = -4176 * i[7] - 4926 * i[5] + 7373 * i[3] + 20995 * i[1]
    return np.stack([descale(wrap32(o), n) for o in (t10 + b, t12 + a, t12 - a, t10 - b)])


def _idct2(i, n):
    i = [wrap32(v) for v in i]
    t10 = i[0] << 15
    t = -5906 * i[7] + 6967 * i[5] - 10426 * i[3] + 29692 * i[1]
    return np.stack([descale(wrap32(o), n) for o in (t10 + t, t10 - t)])


def idct_blocks_reduced(blocks, q, size):
    """(n, 8, 8) coefficients, (8, 8) table -> (n, size, size) samples in [0, 255]."""
    if size == 8:
        return idct_blocks(blocks, q)
    d = np.asarray(blocks, np.int64) * np.asarray(q, np.int64).reshape(1, 8, 8)
    if size == 1:
        return np.clip(wrap32(descale(d[:, :1, :1], 3) + 128), 0, 255)
    one, n1, n2 = (_idct4, 12, 19) if size == 4 else (_idct2, 13, 20)
    ws = one(d.transpose(1, 0, 2), n1)                       # columns: (size, n, 8); unused columns are never read
    px = one(ws.transpose(2, 1, 0), n2)                      # rows: over the column index -> (size col, n, size row)
    return np.clip(wrap32(px.transpose(1, 2, 0) + 128), 0, 255)


def plane_reduced(blocks, q, gr, gc, size, h, w):
    px = idct_blocks_reduced(np.asarray(blocks).reshape(gr * gc, 8, 8), q, size)
    return px.reshape(gr, gc, size, size).transpose(0, 2, 1, 3).reshape(size * gr, size * gc)[:h, :w]


def render_scaled(planar, H, W, mode, qtables, grids, denom):
    if denom == 1:
        from libjpeg_ref import render_coeffs
        return render_coeffs(planar, H, W, mode, qtables, grids)
    assert denom in (2, 4, 8)
    m = 8 // denom
    cf = np.asarray(planar, np.int16).reshape(-1, 64).astype(np.int64)
    q = np.asarray(qtables).reshape(-1, 8, 8)
    oh, ow = -(-H // denom), -(-W // denom)
    gr, gc = grids[0]
    y = plane_reduced(cf[:gr * gc], q[0], gr, gc, m, oh, ow)
    if mode == 'gray':
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    hmax, vmax = SUB[mode]
    s = chroma_size(m, hmax, vmax)
    ux, uy = hmax * m // s, vmax * m // s
    assert uy == 1 and ux in (1, 2), 'h2v2 does not occur at 1/2, 1/4, 1/8'
    ch, cw = -(-H * s // (8 * vmax)), -(-W * s // (8 * hmax))
    c, b0 = [], gr * gc
    for k in (1, 2):
        r, n = grids[k]
        p = plane_reduced(cf[b0:b0 + r * n], q[k], r, n, s, ch, cw)   # cropped before upsampling
        if ux == 2:
            p = upsample_h2v1(p) if m > 1 else np.repeat(p, 2, axis=1)   # (h2v1 itself replicates up to 2 wide)
        c.append(p[:oh, :ow])
        b0 += r * n
    return colour(y, c[0], c[1])
