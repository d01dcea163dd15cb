"""Reference decoder and writer of baseline JPEGs with an interleaved scan
(T.81 A.2.3, B.2.3, F.1.2, F.2.2), built only from oracle/jpeg_entropy.py's
public pieces: what the interleaved tests compare against.

    decode(data) -> dict
        parses DQT, SOF0, DHT, DRI, SOS; decodes one Ns = 3 scan or three
        Ns = 1 scans block by block in MCU order with one DC predictor per
        component (reset at every restart interval).
          'planar'  the cropped coefficients: Y, Cb, Cr, each component's blocks
                    in raster order of its T.81 grid (int16, flat) -- the layout
                    of jds.entropy.decode_jpeg
          'padded'  per component the full MCU-padded grid (rows, cols, 64)
          'grids'   per component (rows, cols) of the T.81 grid
          'qtables' three row-major 8x8 tables, 'tq', 'huff' {(class, id):
                    (bits, vals)}, 'scan_tables' per component (dc id, ac id),
                    'ri', 'H', 'W', 'mode', 'mcu' (rows, cols), 'segment' the
                    entropy-coded bytes of the (first) scan, markers included
    write(padded, H, W, mode, qtables, tq, huff, scan_tables, ri=0) -> bytes
        the interleaved file of MCU-padded grids: SOI DQT.. SOF0 DHT x4 [DRI]
        SOS, MCUs in raster order, every interval padded with 1-bits and
        followed by RSTm, EOI.

The identity that makes the decoder trustworthy on foreign files:
entropy_segment(decode(f)['padded'], f's tables) == f's entropy-coded segment."""
import numpy as np

from oracle import jpeg_entropy as je

MODES = {0x11: '4:4:4', 0x21: '4:2:2', 0x22: '4:2:0'}
STD_HUFF = {(0, 0): je.DC_LUMA, (0, 1): je.DC_CHROMA, (1, 0): je.AC_LUMA, (1, 1): je.AC_CHROMA}
STD_SCAN_TABLES = ((0, 0), (1, 1), (1, 1))


def geometry(H, W, mode):
    """-> (hs, vs) per component, T.81 grids (rows, cols), MCU grid (rows, cols)."""
    hmax, vmax = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}[mode]
    samp = [(hmax, vmax), (1, 1), (1, 1)]
    grids = []
    for hs, vs in samp:
        xc, yc = -(-W * hs // hmax), -(-H * vs // vmax)
        grids.append((-(-yc // 8), -(-xc // 8)))
    mcu = (-(-H // (8 * vmax)), -(-W // (8 * hmax)))
    return samp, grids, mcu


def padded_shapes(H, W, mode):
    samp, _, mcu = geometry(H, W, mode)
    return [(mcu[0] * vs, mcu[1] * hs) for hs, vs in samp]


def mcu_order(H, W, mode):
    """[(component, row, col)] of every block of the interleaved scan, in scan order."""
    samp, _, mcu = geometry(H, W, mode)
    out = []
    for my in range(mcu[0]):
        for mx in range(mcu[1]):
            for c, (hs, vs) in enumerate(samp):
                for by in range(vs):
                    for bx in range(hs):
                        out.append((c, my * vs + by, mx * hs + bx))
    return out


def crop(padded, grids):
    return np.concatenate([np.asarray(p)[:gr, :gc].reshape(-1) for p, (gr, gc) in zip(padded, grids)]).astype(np.int16)


class _Reader(je.BitReader):
    def symbol(self, table):
        code, length = 0, 0
        while True:
            code = (code << 1) | self.bit()
            length += 1
            if (length, code) in table:
                return table[(length, code)]
            assert length < 16, 'bad Huffman code'


def _decode_block(r, dct, act, pred):
    zz = np.zeros(64, np.int64)
    s = r.symbol(dct)
    pred += je._extend(r.bits(s), s)
    zz[0] = pred
    k = 1
    while k < 64:
        rs = r.symbol(act)
        run, s = rs >> 4, rs & 15
        if s == 0:
            if run == 15:
                k += 16
                continue
            break
        k += run
        zz[k] = je._extend(r.bits(s), s)
        k += 1
    out = np.zeros(64, np.int64)
    out[je.ZIGZAG] = zz
    return out, pred


def _split_intervals(seg):
    """The entropy-coded segment cut at its RSTm markers."""
    parts, a, i = [], 0, 0
    while i + 1 < len(seg):
        if seg[i] == 0xFF and 0xD0 <= seg[i + 1] <= 0xD7:
            assert seg[i + 1] == 0xD0 + (len(parts) & 7), 'restart markers out of order'
            parts.append(seg[a:i])
            a = i = i + 2
        else:
            i += 1
    parts.append(seg[a:])
    return parts


def decode(data):
    data = bytes(data)
    assert data[:2] == b'\xff\xd8'
    p, qt, huff, ri, scans = 2, {}, {}, 0, []
    H = W = None
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
            assert seg[0] == 8 and seg[5] == 3
            H, W = int.from_bytes(seg[1:3], 'big'), int.from_bytes(seg[3:5], 'big')
            assert [seg[6], seg[9], seg[12]] == [1, 2, 3] and seg[10] == 0x11 and seg[13] == 0x11
            mode = MODES[seg[7]]
            tq = [seg[8], seg[11], seg[14]]
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
            ns = seg[0]
            comps = [(seg[1 + 2 * i] - 1, seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            assert tuple(seg[1 + 2 * ns:4 + 2 * ns]) == (0, 63, 0)
            e = p
            while not (data[e] == 0xFF and data[e + 1] != 0x00 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            scans.append((comps, data[p:e], ri))
            p = e
    samp, grids, mcu = geometry(H, W, mode)
    shapes = padded_shapes(H, W, mode)
    dec = {k: {(l, c): s for s, (c, l) in je.huffman_codes(t).items()} for k, t in huff.items()}
    scan_tables = [None] * 3
    if len(scans) == 1:
        comps, seg, sri = scans[0]
        assert [c for c, _, _ in comps] == [0, 1, 2]
        padded = [np.zeros(s + (64,), np.int64) for s in shapes]
        for c, td, ta in comps:
            scan_tables[c] = (td, ta)
        order = mcu_order(H, W, mode)
        bpm = sum(hs * vs for hs, vs in samp)
        per = sri * bpm if sri else len(order)
        parts = _split_intervals(seg) if sri else [seg]
        assert len(parts) == -(-len(order) // per)
        for i, part in enumerate(parts):
            r, pred = _Reader(part), [0, 0, 0]
            for c, y, x in order[i * per:(i + 1) * per]:
                td, ta = scan_tables[c]
                padded[c][y, x], pred[c] = _decode_block(r, dec[(0, td)], dec[(1, ta)], pred[c])
            assert r.p == len(part), 'interval holds more bytes than its blocks'
    else:
        assert len(scans) == 3
        # a non-interleaved scan holds exactly its component's T.81 grid
        padded = [np.zeros(g + (64,), np.int64) for g in grids]
        for comps, seg, sri in scans:
            (c, td, ta), = comps
            scan_tables[c] = (td, ta)
            gr, gc = grids[c]
            per = sri if sri else gr * gc
            parts = _split_intervals(seg) if sri else [seg]
            assert len(parts) == -(-(gr * gc) // per)
            for i, part in enumerate(parts):
                r, pred = _Reader(part), 0
                for n in range(i * per, min((i + 1) * per, gr * gc)):
                    padded[c][n // gc, n % gc], pred = _decode_block(r, dec[(0, td)], dec[(1, ta)], pred)
    return {'H': H, 'W': W, 'mode': mode, 'qtables': np.stack([qt[t] for t in tq]), 'tq': tq, 'qt': qt, 'huff': huff,
            'scan_tables': scan_tables, 'ri': scans[0][2], 'grids': grids, 'mcu': mcu, 'interleaved': len(scans) == 1,
            'padded': padded, 'planar': crop(padded, grids), 'segment': scans[0][1]}


# --- writer -----------------------------------------------------------------

def entropy_segment(padded, H, W, mode, huff, scan_tables, ri=0):
    """The interleaved scan's entropy-coded bytes, RSTm markers included."""
    samp, _, _ = geometry(H, W, mode)
    codes = {k: je.huffman_codes(t) for k, t in huff.items()}
    order = mcu_order(H, W, mode)
    bpm = sum(hs * vs for hs, vs in samp)
    per = ri * bpm if ri else len(order)
    zz = [np.asarray(p, np.int64).reshape(p.shape[0], p.shape[1], 64)[:, :, je.ZIGZAG] for p in padded]
    out = bytearray()
    for i, a in enumerate(range(0, len(order), per)):
        if i:
            out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        w, pred = je.BitWriter(), [0, 0, 0]
        for c, y, x in order[a:a + per]:
            td, ta = scan_tables[c]
            b = zz[c][y, x]
            for cls, sym, mag, mlen in je.block_symbols(b, pred[c]):
                code, length = (codes[(0, td)] if cls == 'dc' else codes[(1, ta)])[sym]
                w.put(code, length)
                w.put(mag, mlen)
            pred[c] = int(b[0])
        out += w.flush()
    return bytes(out)


def headers(H, W, mode, qt, tq, huff, ri=0):
    """SOI, DQT per table id in qt ({id: 8x8}), SOF0, DHT x4, DRI when ri."""
    out = bytearray(b'\xff\xd8')
    for i in sorted(qt):
        q = np.asarray(qt[i], np.float64).reshape(64)[je.ZIGZAG]
        out += b'\xff\xdb\x00\x43' + bytes([i]) + bytes(int(v) for v in q)
    out += b'\xff\xc0\x00\x11\x08' + int(H).to_bytes(2, 'big') + int(W).to_bytes(2, 'big') + b'\x03'
    out += bytes([1, je.SAMPLING[mode], tq[0], 2, 0x11, tq[1], 3, 0x11, tq[2]])
    for (tc, th), (bits, vals) in sorted(huff.items()):
        out += b'\xff\xc4' + (3 + 16 + len(vals)).to_bytes(2, 'big') + bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)
    if ri:
        out += b'\xff\xdd\x00\x04' + int(ri).to_bytes(2, 'big')
    return bytes(out)


def sos3(scan_tables):
    return b'\xff\xda\x00\x0c\x03' + bytes(sum(([c + 1, td << 4 | ta] for c, (td, ta) in enumerate(scan_tables)), [])) \
        + bytes([0, 63, 0])


def write(padded, H, W, mode, qt, tq=(0, 1, 1), huff=None, scan_tables=STD_SCAN_TABLES, ri=0):
    huff = STD_HUFF if huff is None else huff
    shapes = padded_shapes(H, W, mode)
    assert [tuple(p.shape[:2]) for p in padded] == shapes, ([p.shape for p in padded], shapes)
    return headers(H, W, mode, qt, tq, huff, ri) + sos3(scan_tables) \
        + entropy_segment(padded, H, W, mode, huff, scan_tables, ri) + b'\xff\xd9'


def random_padded(rng, H, W, mode, amp=40, density=0.3, pad_dc=None):
    """MCU-padded grids of random sparse blocks; padding blocks get non-zero content with
    distinct DCs (pad_dc: alternate +-pad_dc instead)."""
    samp, grids, _ = geometry(H, W, mode)
    out = []
    for c, ((gr, gc), (pr, pc)) in enumerate(zip(grids, padded_shapes(H, W, mode))):
        b = rng.integers(-amp, amp + 1, (pr, pc, 64)) * (rng.random((pr, pc, 64)) < density)
        b[:, :, 0] = rng.integers(-200, 201, (pr, pc))
        pad = np.ones((pr, pc), bool)
        pad[:gr, :gc] = False
        n = int(pad.sum())
        if n:
            b[pad, 1] = rng.integers(1, 30, n)
            b[pad, 0] = (np.where(np.arange(n) % 2, -pad_dc, pad_dc) if pad_dc
                         else 300 + 7 * np.arange(n) * (1 if c != 1 else -1))
        out.append(b.astype(np.int64))
    return out
