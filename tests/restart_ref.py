"""Reference writer of JFIF files with restart intervals (T.81 B.2.4.4, E.1.4),
built only from oracle/jpeg_entropy.py's public functions: the byte-for-byte
definition the restart tests compare against.

    jfif_headers(H, W, mode, qtable)              SOI APP0 DQT SOF0 DHT x4
    + FF DD 00 04 <Ri, big-endian>                DRI, directly after the last DHT
    + for comp in 1, 2, 3:
          sos(comp)
          + for i, chunk in enumerate(chunks of Ri blocks, raster order):
                (FF, D0 + ((i - 1) & 7)  if i > 0)
                + encode_scan(chunk, chroma)[0]   from pred = 0, padded with 1-bits, stuffed
    + FF D9

A non-interleaved scan's MCU is one block, so Ri counts blocks; a scan of at
most Ri blocks holds no marker.  scan_bits of a scan: the sum of the chunks'
entropy-coded bits (pads and markers excluded)."""
import numpy as np

from oracle import jpeg_entropy as je


def counts(h, w, mode):
    ny = ((h + 7) // 8) * ((w + 7) // 8)
    sy, sx = (2, 2) if mode == '4:2:0' else ((1, 2) if mode == '4:2:2' else (1, 1))
    nc = ((h // sy + 7) // 8) * ((w // sx + 7) // 8)
    return ny, nc


def dri(ri):
    return b'\xff\xdd\x00\x04' + bytes([ri >> 8, ri & 255])


def scan_intervals(blocks, chroma, ri):
    """[(stuffed bytes, bits)] of the scan's intervals."""
    return [je.encode_scan(blocks[i:i + ri], chroma) for i in range(0, len(blocks), ri)]


def encode_scan_rst(blocks, chroma, ri):
    """(entropy-coded segment with its RSTm markers, bits, markers)."""
    out, bits = bytearray(), 0
    ivs = scan_intervals(blocks, chroma, ri)
    for i, (seg, nb) in enumerate(ivs):
        if i:
            out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        out += seg
        bits += nb
    return bytes(out), bits, len(ivs) - 1


def encode_jfif_rst(coeffs, H, W, mode, qtable, ri):
    """-> (file, [bits of the Y, Cb, Cr scans], markers in the file)."""
    assert 1 <= ri <= 65535
    ny, nc = counts(H, W, mode)
    blocks = np.asarray(coeffs, np.int16).reshape(-1, 64)
    assert len(blocks) == ny + 2 * nc
    out = bytearray(je.jfif_headers(H, W, mode, qtable)) + dri(ri)
    bits, markers = [], 0
    for comp, (lo, hi) in enumerate(((0, ny), (ny, ny + nc), (ny + nc, ny + 2 * nc)), start=1):
        seg, nb, nm = encode_scan_rst(blocks[lo:hi], comp > 1, ri)
        out += je.sos(comp) + seg
        bits.append(nb)
        markers += nm
    return bytes(out + b'\xff\xd9'), bits, markers


def stuffed_ff_before_marker(data):
    """Occurrences of FF 00 FF Dn (n in 0..7): an interval ending in a stuffed 0xFF."""
    return sum(1 for i in range(len(data) - 3)
               if data[i] == 0xFF and data[i + 1] == 0x00 and data[i + 2] == 0xFF and 0xD0 <= data[i + 3] <= 0xD7)
