"""Reference of the lossless transforms (DESIGN.md "Lossless transforms"), built from
interleaved_ref and transcode_ref in NumPy: the byte-for-byte definition
jds.codec.jpeg_transform and its host model are tested against.

    transform(data, op, trim, optimize) -> bytes
        decode, transform the planar coefficients, edit the header prefix, and write with
        transcode_ref.write at the new H, W and the same mode.
    coef_transform(planar, H, W, mode, op, trim) -> (planar', H', W')

Per component with block grid B[r][c] (R x C) and row-major coefficients k[v][u]:
    hflip      B'[r][C-1-c] = B[r][c],  k'[v][u] = (-1)^u k[v][u]
    vflip      B'[R-1-r][c] = B[r][c],  k'[v][u] = (-1)^v k[v][u]
    transpose  B'[c][r]     = B[r][c],  k'[u][v] = k[v][u]
    rot90 = transpose, then hflip;  rot270 = hflip, then transpose;  rot180 = hflip and vflip;
    transverse = transpose, then rot180.
Negation is int16 arithmetic that wraps (-(-32768) = -32768).
A mirrored source axis must be whole MCUs: NotSupported without trim, with trim the source is
cropped on that axis to whole MCUs first (Empty when nothing is left).  4:2:2 does not
transpose (NotSupported).  'none' (and 'auto' without a usable EXIF Orientation) is
transcode_ref.transcode."""
import numpy as np

import interleaved_ref as il
import transcode_ref as tr
from oracle import jpeg_entropy as je

OPS = ['none', 'hflip', 'vflip', 'transpose', 'transverse', 'rot90', 'rot180', 'rot270']
TRANSPOSING = ('transpose', 'transverse', 'rot90', 'rot270')
MIRRORS_H = ('hflip', 'rot180', 'transverse', 'rot270')        # the source's horizontal axis
MIRRORS_V = ('vflip', 'rot180', 'transverse', 'rot90')
ORIENTATION = {1: 'none', 2: 'hflip', 3: 'rot180', 4: 'vflip', 5: 'transpose', 6: 'rot90', 7: 'transverse',
               8: 'rot270'}
MCU = {'4:4:4': (8, 8), '4:2:2': (8, 16), '4:2:0': (16, 16)}    # rows, columns of samples


class NotSupported(ValueError):
    pass


class Empty(ValueError):
    pass


def _neg(a):
    return (0 - a.astype(np.int32)).astype(np.int16)


_ODD = (np.arange(8) % 2 == 1)


def _hflip(g):
    g = g[:, ::-1].copy()
    g[:, :, :, _ODD] = _neg(g[:, :, :, _ODD])
    return g


def _vflip(g):
    g = g[::-1].copy()
    g[:, :, _ODD, :] = _neg(g[:, :, _ODD, :])
    return g


def _transpose(g):
    return np.ascontiguousarray(g.transpose(1, 0, 3, 2))


_STEPS = {'hflip': [_hflip], 'vflip': [_vflip], 'transpose': [_transpose], 'rot90': [_transpose, _hflip],
          'rot270': [_hflip, _transpose], 'rot180': [_hflip, _vflip], 'transverse': [_transpose, _hflip, _vflip]}


def output_size(H, W, mode, op, trim):
    """(cropped source H, W), (output H, W); raises NotSupported / Empty."""
    mh, mw = MCU[mode]
    if op in TRANSPOSING and mode == '4:2:2':
        raise NotSupported('4:2:2 takes only hflip, vflip and rot180')
    if op in MIRRORS_H and W % mw:
        if not trim:
            raise NotSupported(f'width {W} is not a multiple of {mw}')
        W -= W % mw
    if op in MIRRORS_V and H % mh:
        if not trim:
            raise NotSupported(f'height {H} is not a multiple of {mh}')
        H -= H % mh
    if H < 1 or W < 1:
        raise Empty('trim leaves nothing')
    return (H, W), ((W, H) if op in TRANSPOSING else (H, W))


def coef_transform(planar, H, W, mode, op, trim=False):
    if op == 'none':
        return np.asarray(planar, np.int16).reshape(-1).copy(), H, W
    (cH, cW), (oH, oW) = output_size(H, W, mode, op, trim)
    _, grids, _ = il.geometry(H, W, mode)
    _, cgrids, _ = il.geometry(cH, cW, mode)
    _, ogrids, _ = il.geometry(oH, oW, mode)
    planar = np.asarray(planar, np.int16).reshape(-1)
    out, off = [], 0
    for (gr, gc), (cr, cc), og in zip(grids, cgrids, ogrids):
        g = planar[off:off + 64 * gr * gc].reshape(gr, gc, 8, 8)[:cr, :cc]
        off += 64 * gr * gc
        for step in _STEPS[op]:
            g = step(g)
        assert g.shape[:2] == og, (g.shape, og)
        out.append(g.reshape(-1))
    assert off == planar.size
    return np.concatenate(out).astype(np.int16), oH, oW


def exif_orientation(prefix):
    """(value 1..8, position of its two bytes in the prefix, big-endian?) of the first APP1 Exif
    segment's IFD0 tag 0x0112 (SHORT, count 1), or None."""
    prefix, p = bytes(prefix), 0
    while p + 4 <= len(prefix):
        m, ln = prefix[p + 1], int.from_bytes(prefix[p + 2:p + 4], 'big')
        seg = prefix[p + 4:p + 2 + ln]
        if m == 0xE1 and seg[:6] == b'Exif\x00\x00':
            t = seg[6:]
            if len(t) < 8 or t[:2] not in (b'MM', b'II'):
                return None
            bo = 'big' if t[:2] == b'MM' else 'little'
            if int.from_bytes(t[2:4], bo) != 42:
                return None
            ifd = int.from_bytes(t[4:8], bo)
            if ifd < 8 or ifd + 2 > len(t):
                return None
            n = int.from_bytes(t[ifd:ifd + 2], bo)
            if ifd + 2 + 12 * n > len(t):
                return None
            for i in range(n):
                e = ifd + 2 + 12 * i
                if int.from_bytes(t[e:e + 2], bo) != 0x0112:
                    continue
                if int.from_bytes(t[e + 2:e + 4], bo) != 3 or int.from_bytes(t[e + 4:e + 8], bo) != 1:
                    return None
                v = int.from_bytes(t[e + 8:e + 10], bo)
                return (v, p + 4 + 6 + e + 8, bo == 'big') if 1 <= v <= 8 else None
            return None
        p += 2 + ln
    return None


def edit_prefix(prefix, transposing, H, W):
    """SOF0 gets H x W; with `transposing` every 8-bit DQT table is transposed."""
    out, p = bytearray(prefix), 0
    zz = np.asarray(je.ZIGZAG)
    while p < len(out):
        m, ln = out[p + 1], int.from_bytes(out[p + 2:p + 4], 'big')
        if m == 0xDB and transposing:
            q = p + 4
            while q < p + 2 + ln:
                if out[q] >> 4:
                    raise NotSupported('16-bit DQT')
                t = np.zeros(64, np.uint8)
                t[zz] = np.frombuffer(bytes(out[q + 1:q + 65]), np.uint8)
                out[q + 1:q + 65] = bytes(t.reshape(8, 8).T.reshape(64)[zz])
                q += 65
        elif m == 0xC0:
            out[p + 5:p + 9] = int(H).to_bytes(2, 'big') + int(W).to_bytes(2, 'big')
        p += 2 + ln
    return out


def transform(data, op='auto', trim=False, optimize=True):
    d = il.decode(data)
    prefix, pos = tr.header_prefix(data), None
    if op == 'auto':
        e = exif_orientation(prefix)
        op = ORIENTATION[e[0]] if e else 'none'
        pos = e if e else None
    if op == 'none':
        return tr.write(d['planar'], d['H'], d['W'], d['mode'], prefix, optimize)
    planar, H, W = coef_transform(d['planar'], d['H'], d['W'], d['mode'], op, trim)
    prefix = edit_prefix(prefix, op in TRANSPOSING, H, W)
    if pos:
        prefix[pos[1]:pos[1] + 2] = (1).to_bytes(2, 'big' if pos[2] else 'little')
    return tr.write(planar, H, W, d['mode'], bytes(prefix), optimize)
