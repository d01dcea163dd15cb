"""libjpeg's default rendering of decoded baseline coefficients in NumPy (DESIGN.md "libjpeg
rendering"): what render='libjpeg' is compared against, itself pinned to Pillow byte for byte
(tests/test_jpeg_render_cpu.py).

    render_coeffs(planar, H, W, mode, qtables, grids) -> HxWx3 uint8
        planar: jds.entropy.decode_jpeg's layout (Y, Cb, Cr; each component's blocks in raster
        order of its T.81 grid); mode '4:4:4', '4:2:2', '4:2:0' or 'gray'.
    render(data) -> HxWx3 uint8
        a file, through interleaved_ref.decode / gray_ref.decode.

The steps are jdcoefct's dequantisation, jidctint's ISLOW inverse (CONST_BITS 13, PASS1_BITS 2),
jdsample's fancy upsampling (replication when the chroma plane is at most two samples wide) and
jdcolor's 16-bit fixed-point conversion.  libjpeg computes in `long`; here every value is taken
modulo 2^32 (two's complement) wherever it is shifted or stored, which is what a 32-bit core
computes at every operation, since +, - and * commute with the reduction.  For coefficients below
the bound in DESIGN.md nothing wraps and the two agree."""
import numpy as np

F = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137,
         c1_961=16069, c2_053=16819, c2_562=20995, c3_072=25172)
SUB = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}    # (Hmax, Vmax); chroma is 1 x 1


def wrap32(x):
    """int64 -> the int32 with the same low 32 bits, as int64."""
    return np.asarray(x, np.int64).astype(np.uint64).astype(np.uint32).astype(np.int32).astype(np.int64)


def descale(x, n):
    return wrap32(x + (1 << (n - 1))) >> n


def idct_1d(i, n):
    """One pass over the first axis of i (8, ...), each output DESCALEd by n."""
    i = [wrap32(v) for v in i]
    z1 = (i[2] + i[6]) * F['c0_541']
    tmp2 = z1 - i[6] * F['c1_847']
    tmp3 = z1 + i[2] * F['c0_765']
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F['c1_175']
    a0, a1, a2, a3 = a0 * F['c0_298'], a1 * F['c2_053'], a2 * F['c3_072'], a3 * F['c1_501']
    z1, z2 = z1 * -F['c0_899'], z2 * -F['c2_562']
    z3, z4 = z3 * -F['c1_961'] + z5, z4 * -F['c0_390'] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([descale(wrap32(o), n) for o in out])


def idct_blocks(blocks, q):
    """(n, 8, 8) coefficients, (8, 8) table -> (n, 8, 8) samples in [0, 255]."""
    d = np.asarray(blocks, np.int64) * np.asarray(q, np.int64).reshape(1, 8, 8)
    ws = idct_1d(d.transpose(1, 0, 2), 11)                   # columns: over the row index
    px = idct_1d(ws.transpose(2, 1, 0), 18)                  # rows: over the column index -> (col, n, row)
    return np.clip(wrap32(px.transpose(1, 2, 0) + 128), 0, 255)


def plane(blocks, q, gr, gc, h, w):
    px = idct_blocks(np.asarray(blocks).reshape(gr * gc, 8, 8), q)
    return px.reshape(gr, gc, 8, 8).transpose(0, 2, 1, 3).reshape(8 * gr, 8 * gc)[:h, :w]


def _interleave(even, odd):
    out = np.empty((even.shape[0], 2 * even.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out


def upsample_h2v1(s):
    if s.shape[1] <= 2:
        return np.repeat(s, 2, axis=1)
    p = np.pad(s, ((0, 0), (1, 1)), mode='edge')
    return _interleave((3 * s + p[:, :-2] + 1) >> 2, (3 * s + p[:, 2:] + 2) >> 2)


def upsample_h2v2(s):
    if s.shape[1] <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    pr = np.pad(s, ((1, 1), (0, 0)), mode='edge')
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    for v, other in ((0, pr[:-2]), (1, pr[2:])):             # even output rows: the row above; odd: below
        t = 3 * s + other
        tp = np.pad(t, ((0, 0), (1, 1)), mode='edge')
        out[v::2] = _interleave((3 * t + tp[:, :-2] + 8) >> 4, (3 * t + tp[:, 2:] + 7) >> 4)
    return out


def colour(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def render_coeffs(planar, H, W, mode, qtables, grids):
    cf = np.asarray(planar, np.int16).reshape(-1, 64).astype(np.int64)
    q = np.asarray(qtables).reshape(-1, 8, 8)
    gr, gc = grids[0]
    y = plane(cf[:gr * gc], q[0], gr, gc, H, W)
    if mode == 'gray':
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    hmax, vmax = SUB[mode]
    ch, cw = -(-H // vmax), -(-W // hmax)
    up = {(1, 1): lambda s: s, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(hmax, vmax)]
    c, b0 = [], gr * gc
    for k in (1, 2):
        r, n = grids[k]
        c.append(up(plane(cf[b0:b0 + r * n], q[k], r, n, ch, cw))[:H, :W])   # the T.81 plane, cropped before upsampling
        b0 += r * n
    return colour(y, c[0], c[1])


def decode(data):
    """(planar, H, W, mode, qtables (3, 8, 8), grids) of a colour or one-component file."""
    data = bytes(data)
    sof = data.index(b'\xff\xc0')
    if data[sof + 9] == 1:
        import gray_ref
        d = gray_ref.decode(data)
        q = np.zeros((3, 8, 8))
        q[0] = d['qtable']
        return d['planar'], d['H'], d['W'], 'gray', q, [d['grid'], (0, 0), (0, 0)]
    import interleaved_ref
    d = interleaved_ref.decode(data)
    return d['planar'], d['H'], d['W'], d['mode'], d['qtables'], d['grids']


def render(data):
    return render_coeffs(*decode(data))
