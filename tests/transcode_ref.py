"""Reference of the lossless transcode (DESIGN.md "Transcode"), built from
interleaved_ref, huffopt_ref and oracle/jpeg_entropy.py: the byte-for-byte
definition jds.codec.jpeg_transcode and jds.entropy.encode_jpeg are tested
against.

    transcode(data, optimize) -> bytes
        the file's decoded coefficients on their T.81 grids, unchanged, written
        as ONE interleaved scan (Ns = 3, components 1, 2, 3, Y with tables 0/0,
        Cb and Cr with 1/1, no DRI) behind the input's own header segments:
          SOI | every segment before the first SOS except DHT and DRI, verbatim
              | DHT 0x00, 0x10, 0x01, 0x11 | SOS | scan | EOI
        optimize=False: the Annex K tables; True: K.2/K.3 tables of this scan's
        own symbol counts (huffopt_ref.optimal_table; luma from the Y blocks,
        chroma from Cb and Cr together, padding blocks included).
    The blocks that pad the image to whole MCUs are libjpeg's dummy blocks: AC
    zero, DC = the DC of the preceding block of the same component in scan
    order (0 if a scan could start with one), so each codes as a zero DC
    difference and EOB and the next real block predicts from the last real one.
    A block baseline Huffman coding cannot express (DC difference category
    above 11, AC category above 10) raises NotCodable.
"""
import numpy as np

import huffopt_ref as ho
import interleaved_ref as il
from oracle import jpeg_entropy as je


class NotCodable(ValueError):
    pass


def header_prefix(data):
    """The bytes between SOI and the first SOS, DHT and DRI segments (and fill bytes) left out."""
    data, p, out = bytes(data), 2, bytearray()
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xDA:
            return bytes(out)
        ln = int.from_bytes(data[p + 2:p + 4], 'big')
        if m not in (0xC4, 0xDD):
            out += data[p:p + 2 + ln]
        p += 2 + ln


def dummy_padded(planar, H, W, mode):
    """Cropped planar coefficients -> MCU-padded grids (rows, cols, 64) with libjpeg's dummy blocks."""
    _, grids, _ = il.geometry(H, W, mode)
    planar = np.asarray(planar, np.int64).reshape(-1)
    padded, off = [], 0
    for (gr, gc), (pr, pc) in zip(grids, il.padded_shapes(H, W, mode)):
        p = np.zeros((pr, pc, 64), np.int64)
        p[:gr, :gc] = planar[off:off + 64 * gr * gc].reshape(gr, gc, 64)
        off += 64 * gr * gc
        padded.append(p)
    assert off == planar.size, 'coefficient count does not match the T.81 grids'
    last = [0, 0, 0]
    for c, y, x in il.mcu_order(H, W, mode):
        if y < grids[c][0] and x < grids[c][1]:
            last[c] = int(padded[c][y, x, 0])
        else:
            padded[c][y, x, 0] = last[c]
    return padded


def scan_histograms(padded, H, W, mode):
    """{'dc0', 'ac0', 'dc1', 'ac1'} -> counts[256] of the interleaved scan's symbols."""
    h = {k: np.zeros(256, np.int64) for k in ho.CLASSES}
    pred = [0, 0, 0]
    zz = [p[:, :, je.ZIGZAG] for p in padded]
    for c, y, x in il.mcu_order(H, W, mode):
        b = zz[c][y, x]
        for cls, sym, _, _ in je.block_symbols(b, pred[c]):
            if (cls == 'dc' and sym > 11) or (cls == 'ac' and (sym & 15) > 10):
                raise NotCodable('not baseline-codable: %s category %d' % (cls.upper(), sym & 15 if cls == 'ac' else sym))
            h[cls + ('1' if c else '0')][sym] += 1
        pred[c] = int(b[0])
    return h


def scan_tables(padded, H, W, mode, optimize):
    """-> ({(class, id): (BITS, HUFFVAL)}, histograms); raises NotCodable."""
    h = scan_histograms(padded, H, W, mode)
    if not optimize:
        return dict(il.STD_HUFF), h
    t = {k: ho.optimal_table(v, ho.STD[k]) for k, v in h.items()}
    return {(int(k[0] == 'a'), int(k[2])): (list(t[k][0]), list(t[k][1])) for k in ho.CLASSES}, h


def write(planar, H, W, mode, prefix, optimize):
    """SOI + prefix + DHT x4 + SOS + the interleaved scan of the cropped coefficients + EOI."""
    padded = dummy_padded(planar, H, W, mode)
    huff, _ = scan_tables(padded, H, W, mode, optimize)
    out = bytearray(b'\xff\xd8') + bytes(prefix)
    for k in ho.CLASSES:
        bits, vals = huff[(int(k[0] == 'a'), int(k[2]))]
        out += ho.dht(ho.TC_TH[k], bits, vals)
    out += il.sos3(il.STD_SCAN_TABLES)
    out += il.entropy_segment(padded, H, W, mode, huff, il.STD_SCAN_TABLES, 0)
    return bytes(out + b'\xff\xd9')


def transcode(data, optimize):
    d = il.decode(data)
    return write(d['planar'], d['H'], d['W'], d['mode'], header_prefix(data), optimize)


def default_prefix(H, W, mode, qtables, tq):
    """What encode_jpeg writes without a prefix: APP0, one DQT per table id in use, SOF0."""
    out = bytearray(b'\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    done = []
    for c in range(3):
        if tq[c] in done:
            continue
        done.append(tq[c])
        q = np.asarray(qtables[c], np.float64).reshape(64)[je.ZIGZAG]
        out += b'\xff\xdb\x00\x43' + bytes([tq[c]]) + bytes(int(v) for v in q)
    out += b'\xff\xc0\x00\x11\x08' + int(H).to_bytes(2, 'big') + int(W).to_bytes(2, 'big') + b'\x03'
    out += bytes([1, je.SAMPLING[mode], tq[0], 2, 0x11, tq[1], 3, 0x11, tq[2]])
    return bytes(out)
