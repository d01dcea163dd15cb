"""Reference writer of JFIF files with per-frame optimised Huffman tables, built
only from oracle/jpeg_entropy.py's public functions: the byte-for-byte definition
the optimised-table tests compare against (DESIGN.md "Optimised tables").

    histograms    DC luma, AC luma (the Y scan), DC chroma, AC chroma (Cb and Cr
                  together); the symbols of je.block_symbols, DC differences along
                  each scan from pred 0 (restart files: from 0 at every interval)
    table         T.81 K.2 with libjpeg's tie rules, then K.3 (optimal_table)
    file          SOI APP0 DQT SOF0 as je.jfif_headers writes them, four DHT
                  segments (0x00, 0x10, 0x01, 0x11), DRI for a restart file, the
                  three scans coded with the frame's tables, EOI

The K.2 rule: freq[256] = 1 (the reserved symbol: no code is all ones); repeat:
c1 = the index of the smallest non-zero freq, the LARGEST index on a tie, c2 the
same over the other indices; merge c2 into c1, one more bit for every symbol of
both chains.  A code longer than 32 bits: the table falls back to its Annex K
table.  K.3 shortens codes longer than 16 bits; HUFFVAL lists the counted symbols
by their length before K.3, ascending symbol value within a length."""
import heapq

import numpy as np

from oracle import jpeg_entropy as je

CLASSES = ('dc0', 'ac0', 'dc1', 'ac1')                 # the DHT order of the file
TC_TH = {'dc0': 0x00, 'ac0': 0x10, 'dc1': 0x01, 'ac1': 0x11}
STD = {'dc0': je.DC_LUMA, 'ac0': je.AC_LUMA, 'dc1': je.DC_CHROMA, 'ac1': je.AC_CHROMA}


def counts(h, w, mode):
    ny = ((h + 7) // 8) * ((w + 7) // 8)
    sy, sx = (2, 2) if mode == '4:2:0' else ((1, 2) if mode == '4:2:2' else (1, 1))
    nc = ((h // sy + 7) // 8) * ((w // sx + 7) // 8)
    return ny, nc


def code_sizes(freq):
    """K.2 (libjpeg's jpeg_gen_optimal_table): codesize[0..256] before any limiting."""
    f = [int(v) for v in freq] + [1]
    assert len(f) == 257 and min(f) >= 0
    size, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if f[i] and (v is None or f[i] <= v):
                v, c1 = f[i], i
        c2, v = -1, None
        for i in range(257):
            if f[i] and i != c1 and (v is None or f[i] <= v):
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    return size


def unconstrained_length(freq):
    """The longest code K.2 gives before K.3 (the reserved symbol included)."""
    return max(code_sizes(freq))


def limit_bits(bits):
    """K.3 on bits[0..32] in place (Adjust_BITS), the reserved code taken off."""
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1
    return bits


def optimal_table(freq, std=je.AC_LUMA):
    """freq[0..255] -> (BITS[1..16], HUFFVAL, fell_back).  std: the Annex K table of this
    class, returned when a code would exceed 32 bits."""
    size = code_sizes(freq)
    if max(size) > 32:
        return list(std[0]), list(std[1]), True
    bits = [0] * 33
    for s in size:
        if s:
            bits[s] += 1
    limit_bits(bits)
    vals = [i for s in range(1, 33) for i in range(256) if size[i] == s]
    assert sum(bits[1:17]) == len(vals) and not any(bits[17:])
    return bits[1:17], vals, False


def plain_huffman_cost(freq):
    """Total bits of an unconstrained Huffman code over freq + [1], the reserved symbol's code
    included (every Huffman code of a histogram has this cost, whatever its ties do): what
    optimal_table must cost wherever K.3 does not act."""
    f = [int(v) for v in freq]
    heap = [(v, i, (i,)) for i, v in enumerate(f + [1]) if v]
    heapq.heapify(heap)
    depth = [0] * 257
    n = 257
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for i in a[2] + b[2]:
            depth[i] += 1
        heapq.heappush(heap, (a[0] + b[0], n, a[2] + b[2]))
        n += 1
    return sum(f[i] * depth[i] for i in range(256)) + depth[256]


def table_cost(freq, table):
    codes = je.huffman_codes(table)
    return sum(int(v) * codes[i][1] for i, v in enumerate(freq) if v)


def _scan_chunks(blocks, ri):
    return [blocks[i:i + ri] for i in range(0, len(blocks), ri)] if ri else [blocks]


def histograms(coeffs, H, W, mode, ri=0):
    """{'dc0', 'ac0', 'dc1', 'ac1'} -> counts[256] of the frame's symbols."""
    ny, nc = counts(H, W, mode)
    blocks = np.asarray(coeffs, np.int64).reshape(-1, 64)[:, je.ZIGZAG]
    assert len(blocks) == ny + 2 * nc
    h = {k: np.zeros(256, np.int64) for k in CLASSES}
    for comp, (lo, hi) in enumerate(((0, ny), (ny, ny + nc), (ny + nc, ny + 2 * nc))):
        c = '1' if comp else '0'
        for chunk in _scan_chunks(blocks[lo:hi], ri):
            pred = 0
            for b in chunk:
                for cls, sym, _, _ in je.block_symbols(b, pred):
                    h[cls + c][sym] += 1
                pred = int(b[0])
    return h


def frame_tables(coeffs, H, W, mode, ri=0):
    """{'dc0', ...} -> (BITS, HUFFVAL, fell_back) of the frame."""
    return {k: optimal_table(v, STD[k]) for k, v in histograms(coeffs, H, W, mode, ri).items()}


def dht(tc_th, bits, vals):
    return b'\xff\xc4' + (19 + len(vals)).to_bytes(2, 'big') + bytes([tc_th]) + bytes(bits) + bytes(vals)


def headers(H, W, mode, qtable, tables):
    std = je.jfif_headers(H, W, mode, qtable)
    n_std = sum(5 + 16 + len(t[1]) for t in STD.values())
    out = bytearray(std[:len(std) - n_std])          # SOI APP0 DQT SOF0
    for k in CLASSES:
        out += dht(TC_TH[k], tables[k][0], tables[k][1])
    return bytes(out)


def encode_chunk(blocks, dc, ac):
    """One scan or interval with the given code maps -> (stuffed bytes, bits)."""
    w = je.BitWriter()
    pred = 0
    for b in np.asarray(blocks, np.int64).reshape(-1, 64)[:, je.ZIGZAG]:
        for cls, sym, mag, mlen in je.block_symbols(b, pred):
            code, length = (dc if cls == 'dc' else ac)[sym]
            w.put(code, length)
            w.put(mag, mlen)
        pred = int(b[0])
    bits = w.bits
    return w.flush(), bits


def encode_jfif_opt(coeffs, H, W, mode, qtable, ri=0):
    """-> (file, [bits of the Y, Cb, Cr scans], the frame's tables)."""
    ny, nc = counts(H, W, mode)
    blocks = np.asarray(coeffs, np.int16).reshape(-1, 64)
    assert len(blocks) == ny + 2 * nc
    tabs = frame_tables(blocks, H, W, mode, ri)
    codes = {k: je.huffman_codes((t[0], t[1])) for k, t in tabs.items()}
    out = bytearray(headers(H, W, mode, qtable, tabs))
    if ri:
        out += b'\xff\xdd\x00\x04' + bytes([ri >> 8, ri & 255])
    bits = []
    for comp, (lo, hi) in enumerate(((0, ny), (ny, ny + nc), (ny + nc, ny + 2 * nc)), start=1):
        c = '1' if comp > 1 else '0'
        out += je.sos(comp)
        nb = 0
        for i, chunk in enumerate(_scan_chunks(blocks[lo:hi], ri)):
            if i:
                out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
            seg, n = encode_chunk(chunk, codes['dc' + c], codes['ac' + c])
            out += seg
            nb += n
        bits.append(nb)
    return bytes(out + b'\xff\xd9'), bits, tabs


def file_tables(data):
    """The DHT tables of a file -> {'dc0', ...: (BITS, HUFFVAL)}."""
    data, p, out = bytes(data), 2, {}
    while data[p + 1] != 0xDA:
        ln = int.from_bytes(data[p + 2:p + 4], 'big')
        if data[p + 1] == 0xC4:
            seg, q = data[p + 4:p + 2 + ln], 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                out[('dc', 'ac')[seg[q] >> 4] + str(seg[q] & 15)] = (bits, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        p += 2 + ln
    return out


# --- histograms by name and coefficient sets with prescribed histograms ------

def fibonacci(n):
    """1, 2, 3, 5, ... on symbols 0..n-1."""
    f, a, b = np.zeros(256, np.int64), 1, 2
    for i in range(n):
        f[i] = a
        a, b = b, a + b
    return f


def histogram_cases():
    """{name: freq[256]}: the named and the seeded random histograms the table tests share."""
    out = {f'fibonacci{n}': fibonacci(n) for n in (17, 18, 24, 32, 33)}
    one = np.zeros(256, np.int64)
    one[0x21] = 7
    out['single'] = one
    out['equal256'] = np.full(256, 3, np.int64)
    out['equal255'] = np.concatenate([np.full(255, 1, np.int64), [0]])
    two = np.zeros(256, np.int64)
    two[[0, 255]] = 1
    out['ends'] = two
    rng = np.random.default_rng(20261019)
    for i in range(24):
        f = np.zeros(256, np.int64)
        k = int(rng.integers(1, 257))
        idx = rng.choice(256, k, replace=False)
        kind = i % 4
        if kind == 0:      # flat counts with many ties
            f[idx] = rng.integers(1, 4, k)
        elif kind == 1:    # wide range
            f[idx] = rng.integers(1, 1 << 20, k)
        elif kind == 2:    # geometric: deep trees, K.3 acts once k is large enough
            f[idx] = np.maximum(1, (1.7 ** np.minimum(np.arange(k), 38) * rng.uniform(0.8, 1.2, k))).astype(np.int64)
        else:              # like an AC table: a few heavy symbols and a long tail of ones
            f[idx] = np.where(rng.random(k) < 0.15, rng.integers(100, 100000, k), 1)
        out[f'random{i}'] = f
    return out


def blocks_with_ac_histogram(nblocks, hist):
    """(nblocks, 64) int16 row-major blocks, DC 0, whose AC symbols (je.block_symbols) have
    exactly the counts hist: {symbol: count}.  Symbols are (run << 4 | size) with size in
    1..10, and 0x00 (EOB); ZRL is not supported.  nblocks - hist[EOB] blocks are filled to
    position 63 exactly (they carry no EOB), the others end below it."""
    hist = {int(k): int(v) for k, v in hist.items() if v}
    assert 0xF0 not in hist and all(k == 0 or 1 <= (k & 15) <= 10 for k in hist)
    n_eob = hist.pop(0x00, 0)
    n_full = nblocks - n_eob
    assert n_full >= 0, 'more EOBs than blocks'
    items = sorted(((s >> 4) + 1, s) for s, c in hist.items() for _ in range(c))  # (positions, symbol), short first
    zz = np.zeros((nblocks, 64), np.int64)

    def put(b, pos, sym, k):
        pos += sym >> 4
        zz[b, pos] = (1 << ((sym & 15) - 1)) * (1 if k & 1 else -1)
        return pos + 1

    k = 0
    for b in range(n_full):                          # long items first, one-position items to finish
        pos = 1
        while pos < 64:
            room = 64 - pos
            j = next((i for i in range(len(items) - 1, -1, -1) if items[i][0] <= room and
                      (room - items[i][0] == 0 or room - items[i][0] >= items[0][0])), None)
            assert j is not None, 'cannot fill a block to position 63 with these symbols'
            pos = put(b, pos, items.pop(j)[1], k)
            k += 1
    fill = [1] * n_eob
    b = 0
    while items:
        assert n_eob, 'symbols left and no block with an EOB'
        cost, sym = items.pop()
        for _ in range(n_eob):
            if fill[b] + cost <= 63:                 # the last coefficient stays below position 63
                break
            b = (b + 1) % n_eob
        else:
            raise AssertionError('the histogram does not fit the blocks')
        fill[b] = put(n_full + b, fill[b], sym, k)
        k += 1
        b = (b + 1) % n_eob
    out = np.zeros((nblocks, 64), np.int16)
    out[:, je.ZIGZAG] = zz
    return out


def steep_ac_histogram(counts_desc, n_eob_index):
    """Counts (any order) onto AC symbols: the count at n_eob_index goes to EOB, the largest
    others to the one-position symbols (run 0, sizes 1..10), the rest to run 1, 2, ..."""
    counts_desc = [int(c) for c in counts_desc]
    hist = {0x00: counts_desc[n_eob_index]}
    rest = sorted((c for i, c in enumerate(counts_desc) if i != n_eob_index), reverse=True)
    syms = [(r << 4) | s for r in range(16) for s in range(1, 11)]
    for c, s in zip(rest, syms):
        hist[s] = c
    return hist
