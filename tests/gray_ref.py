"""Reference reader of one-component (grayscale) baseline JPEGs and the cases the
grayscale tests share.  The reader is T.81 F.2 over the file's own DHT, built from
interleaved_ref's bit reader and block decoder and oracle/jpeg_entropy.py's tables --
independent of the C code.

    decode(data) -> dict
        'H', 'W', 'id' (the component id as written), 'sampling' (the SOF0 byte, which does
        not change the geometry: a one-component scan is never interleaved, T.81 A.2.2),
        'tq', 'qtable' (8x8, row-major), 'huff', 'tables' (dc id, ac id), 'ri' (in blocks),
        'grid' (rows, cols) = ceil(H/8) x ceil(W/8), 'planar' (int16, flat: the blocks in
        raster order of the grid), 'segment'.
    oracle_image(planar, H, W, qtable, grid) -> H x W x 3 uint8
        the per-stage definition with the oracle's stages: dequantise, the exact IDCT,
        +128, clip, crop, truncate; each channel is that byte (the colour expressions at
        Cb = Cr = 128 give Y + c * 0.0 = Y).
    pillow_gray(h, w, seed=0, **save) -> bytes
        a Pillow 'L' file of a fixed picture (a gradient plus noise, both ends of the range).
"""
import functools
import io

import numpy as np

import interleaved_ref as ir
from oracle import cpu_ref
from oracle import jpeg_entropy as je


def decode(data):
    data = bytes(data)
    assert data[:2] == b'\xff\xd8'
    p, qt, huff, ri, scan = 2, {}, {}, 0, None
    H = W = cid = smp = tq = None
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xD9:
            break
        ln = int.from_bytes(data[p + 2:p + 4], 'big')
        seg = data[p + 4:p + 2 + ln]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                t = np.zeros(64)
                t[je.ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[seg[q] & 15] = t.reshape(8, 8)
                q += 65
        elif m == 0xC0:
            assert seg[0] == 8 and seg[5] == 1 and len(seg) == 9
            H, W = int.from_bytes(seg[1:3], 'big'), int.from_bytes(seg[3:5], 'big')
            cid, smp, tq = seg[6], seg[7], seg[8]
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                huff[(seg[q] >> 4, seg[q] & 15)] = (bits, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            ri = int.from_bytes(seg[0:2], 'big')
        else:
            assert m == 0xDA or 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
        p += 2 + ln
        if m == 0xDA:
            assert scan is None and seg[0] == 1 and seg[1] == cid and tuple(seg[3:6]) == (0, 63, 0)
            e = p
            while not (data[e] == 0xFF and data[e + 1] != 0x00 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            scan = ((seg[2] >> 4, seg[2] & 15), data[p:e], ri)
            p = e
    (td, ta), seg, sri = scan
    gr, gc = -(-H // 8), -(-W // 8)
    dec = {k: {(l, c): s for s, (c, l) in je.huffman_codes(t).items()} for k, t in huff.items()}
    blocks = np.zeros((gr * gc, 64), np.int64)
    per = sri if sri else gr * gc
    parts = ir._split_intervals(seg) if sri else [seg]
    assert len(parts) == -(-(gr * gc) // per)
    for i, part in enumerate(parts):
        r, pred = ir._Reader(part), 0
        for n in range(i * per, min((i + 1) * per, gr * gc)):
            blocks[n], pred = ir._decode_block(r, dec[(0, td)], dec[(1, ta)], pred)
    return {'H': H, 'W': W, 'id': cid, 'sampling': smp, 'tq': tq, 'qtable': qt[tq], 'huff': huff, 'tables': (td, ta),
            'ri': sri, 'grid': (gr, gc), 'planar': blocks.reshape(-1).astype(np.int16), 'segment': seg}


def oracle_image(planar, H, W, qtable, grid):
    gr, gc = grid
    blocks = np.asarray(planar, np.int16).reshape(gr * gc, 8, 8)
    px = cpu_ref.decode_blocks(cpu_ref.dequantize(blocks, np.asarray(qtable, np.float64).reshape(8, 8)))
    y = np.clip(cpu_ref.merge_blocks(px, (8 * gr, 8 * gc))[:H, :W], 0, 255).astype(np.uint8)
    return np.repeat(y[:, :, None], 3, axis=2)


def picture(h, w, seed=0):
    rng = np.random.default_rng([seed, h, w])
    yy, xx = np.mgrid[0:h, 0:w]
    a = (yy * 5 + xx * 3) % 256 + rng.integers(-60, 61, (h, w)) * (rng.random((h, w)) < 0.5)
    a[:max(1, h // 5)] = np.where(rng.random((max(1, h // 5), w)) < 0.5, 0, 255)    # both ends of the range
    return np.clip(a, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pillow_gray(h, w, seed=0, **save):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture(h, w, seed), 'L').save(buf, 'JPEG', **{'quality': 85, **save})
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def pillow_colour(h, w, subsampling, seed=0):
    from PIL import Image
    rng = np.random.default_rng([seed, h, w, 3])
    a = np.clip(np.stack([picture(h, w, seed + k) for k in range(3)], -1).astype(int) + rng.integers(-9, 10, (h, w, 3)),
                0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a, 'RGB').save(buf, 'JPEG', quality=80, subsampling=subsampling)
    return buf.getvalue()


# every file the parse / decode / render tests run: name -> (h, w, Pillow's save arguments)
FILES = {
    '1x1': (1, 1, {}),
    '8x8': (8, 8, {}),
    '9x9': (9, 9, {}),
    '37x53': (37, 53, {}),
    '40x136': (40, 136, {}),
    '37x53-0x22': (37, 53, {'subsampling': 2}),
    '37x53-opt': (37, 53, {'optimize': True}),
    '40x136-opt': (40, 136, {'optimize': True}),
    '37x53-ri2': (37, 53, {'restart_marker_blocks': 2}),
    '40x136-rows1': (40, 136, {'restart_marker_rows': 1}),
}


def file(name):
    h, w, save = FILES[name]
    return pillow_gray(h, w, 0, **save)


def truncated_scan(data):
    """The file with the second half of its scan data cut away (the headers and EOI stay): a
    defective scan, not an unparseable file."""
    d = decode(data)
    a = bytes(data).index(d['segment'])
    return bytes(data)[:a + len(d['segment']) // 2] + b'\xff\xd9'


def mix():
    """The batch of the CPU and GPU tests: gray, 4:2:0, gray 0x22, 4:4:4, a gray file with a
    truncated scan, an unparseable file."""
    return [file('40x136'), pillow_colour(37, 53, 2), file('37x53-0x22'), pillow_colour(9, 9, 0),
            truncated_scan(pillow_gray(33, 47, 1)), b'\xff\xd8\xff\xe0\x00\x02not a jpeg']


def with_sos(data, sos_payload, tail=None):
    """The file with its SOS segment's payload replaced (the scan data stay)."""
    data = bytes(data)
    a = data.index(b'\xff\xda')
    ln = int.from_bytes(data[a + 2:a + 4], 'big')
    return data[:a] + b'\xff\xda' + (len(sos_payload) + 2).to_bytes(2, 'big') + bytes(sos_payload) + data[a + 2 + ln:]


@functools.lru_cache(maxsize=None)
def long_file():
    """A noisy 'L' file without restart markers whose scan spans more than two workgroups of
    the decoder and takes at least two rounds on the host model (enlarged until it does)."""
    from PIL import Image
    from jds import entropy
    s_bits, g = entropy.decode_info()
    h, w = 200, 264
    while True:
        a = np.random.default_rng([h, w]).integers(0, 256, (h, w)).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a, 'L').save(buf, 'JPEG', quality=95)
        data = buf.getvalue()
        length = entropy.parse_jpeg(data)['scans'][0]['length']
        if 8 * length > 2 * g * s_bits and entropy.host_decode_jpeg(data, s_bits)[1][0] >= 2:
            return data
        h, w = h + 64, w + 64
        assert h < 1200


# --- writer (the byte-for-byte definition of the one-component file form) -------------------

def histograms(planar):
    """{'dc0', 'ac0'} -> counts[256] of the scan's symbols (blocks in raster order, one DC
    predictor); raises transcode_ref.NotCodable."""
    import transcode_ref as tr
    h = {'dc0': np.zeros(256, np.int64), 'ac0': np.zeros(256, np.int64)}
    pred = 0
    for b in np.asarray(planar, np.int64).reshape(-1, 64)[:, je.ZIGZAG]:
        for cls, sym, _, _ in je.block_symbols(b, pred):
            if (cls == 'dc' and sym > 11) or (cls == 'ac' and (sym & 15) > 10):
                raise tr.NotCodable('not baseline-codable: %s category %d' % (cls.upper(), sym & 15 if cls == 'ac' else sym))
            h[cls + '0'][sym] += 1
        pred = int(b[0])
    return h


def write(planar, prefix, optimize, comp_id=1):
    """SOI | prefix | DHT 0x00 | DHT 0x10 | SOS (Ns = 1, the frame's id, tables 0/0) | scan | EOI:
    what libjpeg / Pillow write.  optimize: K.2/K.3 tables of the scan's own counts."""
    import huffopt_ref as ho
    h = histograms(planar)
    huff = {}
    for k in ('dc0', 'ac0'):
        key = (int(k[0] == 'a'), 0)
        if optimize:
            t = ho.optimal_table(h[k], ho.STD[k])
            huff[key] = (list(t[0]), list(t[1]))
        else:
            huff[key] = ir.STD_HUFF[key]
    out = bytearray(b'\xff\xd8') + bytes(prefix)
    for k in ('dc0', 'ac0'):
        out += ho.dht(ho.TC_TH[k], *huff[(int(k[0] == 'a'), 0)])
    out += b'\xff\xda\x00\x08\x01' + bytes([comp_id, 0x00, 0x00, 0x3F, 0x00])
    codes = {k: je.huffman_codes(t) for k, t in huff.items()}
    w, pred = je.BitWriter(), 0
    for b in np.asarray(planar, np.int64).reshape(-1, 64)[:, je.ZIGZAG]:
        for cls, sym, mag, mlen in je.block_symbols(b, pred):
            code, length = codes[(0, 0) if cls == 'dc' else (1, 0)][sym]
            w.put(code, length)
            w.put(mag, mlen)
        pred = int(b[0])
    return bytes(out + w.flush() + b'\xff\xd9')


def default_prefix(H, W, qtable, tq=0):
    """What encode_jpeg writes for mode 'gray' without a prefix: APP0, one DQT, SOF0 with
    Nf = 1, id 1, sampling 0x11."""
    q = np.asarray(qtable, np.float64).reshape(64)[je.ZIGZAG]
    return (b'\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00' + b'\xff\xdb\x00\x43' + bytes([tq])
            + bytes(int(v) for v in q) + b'\xff\xc0\x00\x0b\x08' + int(H).to_bytes(2, 'big') + int(W).to_bytes(2, 'big')
            + bytes([1, 1, 0x11, tq]))


def transcode(data, optimize):
    import transcode_ref as tr
    d = decode(data)
    return write(d['planar'], tr.header_prefix(data), optimize, d['id'])


def info_of(H, W, qtable, tq=0):
    """encode_jpeg's info dict of a gray frame."""
    q = np.zeros((3, 8, 8))
    q[0] = qtable
    return {'H': H, 'W': W, 'mode': 'gray', 'grids': [(-(-H // 8), -(-W // 8)), (0, 0), (0, 0)], 'qtables': q,
            'tq': [tq, 0, 0]}


def extreme_coeffs(H, W, dc_cat=11, ac_cat=10):
    """Blocks that reach a DC difference of category dc_cat and an AC value of category ac_cat,
    all-zero blocks between them."""
    n = -(-H // 8) * -(-W // 8)
    cf = np.zeros((n, 64), np.int64)
    hi = (1 << dc_cat) - 1                      # the largest difference of that category
    cf[0, 0] = -(hi // 2)
    if n > 1:
        cf[1, 0] = cf[0, 0] + hi
        cf[1, 63] = -((1 << ac_cat) - 1)
        cf[1, 5] = 1 << (ac_cat - 1)
    else:
        cf[0, 0] = hi
        cf[0, 63] = -((1 << ac_cat) - 1)
    if n > 3:
        cf[3, 0] = cf[1, 0] - hi                # from +max down by a category-dc_cat difference, over a zero block's DC
        cf[2, 0] = cf[1, 0]
        cf[3, 17] = (1 << ac_cat) - 1
    return cf.reshape(-1).astype(np.int16)


# --- transforms -------------------------------------------------------------------------------

def transform(data, op='auto', trim=False, optimize=True):
    """transform_ref.transform for a one-component file: the same block permutation, in-block
    transpose and signs on the single plane, MCU 8 x 8 whatever the sampling byte says."""
    import transcode_ref as tr
    import transform_ref as xr
    d = decode(data)
    prefix, pos = tr.header_prefix(data), None
    if op == 'auto':
        e = xr.exif_orientation(prefix)
        op = xr.ORIENTATION[e[0]] if e else 'none'
        pos = e if e else None
    if op == 'none':
        return write(d['planar'], prefix, optimize, d['id'])
    H, W = d['H'], d['W']
    if op in xr.MIRRORS_H and W % 8:
        if not trim:
            raise xr.NotSupported(f'width {W} is not a multiple of 8')
        W -= W % 8
    if op in xr.MIRRORS_V and H % 8:
        if not trim:
            raise xr.NotSupported(f'height {H} is not a multiple of 8')
        H -= H % 8
    if H < 1 or W < 1:
        raise xr.Empty('trim leaves nothing')
    gr, gc = d['grid']
    g = d['planar'].reshape(gr, gc, 8, 8)[:-(-H // 8), :-(-W // 8)]
    for step in xr._STEPS[op]:
        g = step(g)
    oH, oW = (W, H) if op in xr.TRANSPOSING else (H, W)
    assert g.shape[:2] == (-(-oH // 8), -(-oW // 8))
    prefix = xr.edit_prefix(prefix, op in xr.TRANSPOSING, oH, oW)
    if pos:
        prefix[pos[1]:pos[1] + 2] = (1).to_bytes(2, 'big' if pos[2] else 'little')
    return write(g.reshape(-1), bytes(prefix), optimize, d['id'])


def with_exif_orientation(data, value):
    """The file with an APP1 Exif segment (big-endian TIFF, IFD0 holding Orientation = value)
    after its first segment."""
    data = bytes(data)
    tiff = b'MM\x00\x2a\x00\x00\x00\x08' + b'\x00\x01' + b'\x01\x12\x00\x03\x00\x00\x00\x01' + int(value).to_bytes(2, 'big') \
        + b'\x00\x00' + b'\x00\x00\x00\x00'
    body = b'Exif\x00\x00' + tiff
    seg = b'\xff\xe1' + (len(body) + 2).to_bytes(2, 'big') + body
    p = 2 + 2 + int.from_bytes(data[4:6], 'big')
    return data[:p] + seg + data[p:]
