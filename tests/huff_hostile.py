"""Hostile Huffman tables and 0xFF-dense scans for the decode core (csrc/jds_huffdec.hpp:
hd_build, hd_window, hd_run) and the device byte sources (DecLdsSrc, RstRowSrc).  A helper,
not collected: tests/test_huff_tables_cpu.py and tests/test_gpu_huff_tables.py use it.

Table families, each a (BITS, HUFFVAL) pair per class (0: DC, 1: AC), checked here against
Kraft's inequality:

    ladder8    [1]*7 + [2]: complete, nine symbols, the all-ones 8-bit code in use
    ladder16   [1]*15 + [2]: complete, the frequent symbols on the 15- and 16-bit codes
    ladder16ff the same lengths with run 0 / size 10 on the all-ones 16-bit code
    gap        codes of 2..8 and of 13..16 bits, none of 9..12 (incomplete)
    flat8      256 symbols, as flat as a DHT can say it: a length count is one byte, so 256
               codes of 8 bits cannot be written; one of 7, 253 of 8 and two of 9 bits is the
               complete 256-symbol code nearest to it (every LUT entry filled, the all-ones
               9-bit code in use)
    random     seeded random lengths, complete or not, random symbol order

Streams fill MCU-padded grids like interleaved_ref.random_padded, from the symbols the
file's tables hold: AC within +-1023, DC values so far inside the largest category of the DC
table that every difference (in any scan order, from 0 after a restart) has a code.

    ff_dense      every AC coefficient 255 on the all-ones code, DC alternating 255 / 0
    ff_mixed      blocks between no and all coefficients 255: every count of 0xFF among five
                  consecutive data bytes occurs (ff_window_histogram)
    ff_dense10,   the same with 1023 on ladder16ff's 16-bit all-ones code and DC differences of
    ff_mixed10    +-2047.  A ladder8 symbol is at most 16 bits and touches three data bytes, so
                  hd_run never needs the window's last two there; these symbols are 26 and 27
                  bits at every bit offset and need all five bytes and all four ffm bits.
    long_codes    +-1 after zero runs of random length, EOB
    sparse_random any symbol the tables hold

Expected coefficients are always the written ones (interleaved_ref.crop)."""
import functools

import numpy as np

import interleaved_ref as ir
from oracle import cpu_ref
from oracle import jpeg_entropy as je

Q50 = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50)
QC = np.clip(Q50 * 2 + 3, 1, 255)
MODES = ['4:2:0', '4:2:2', '4:4:4']

AC_ALL = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]      # baseline's 162
AC_L8 = [0x00, 0x01, 0x11, 0x02, 0x03, 0x04, 0xF0, 0x07, 0x08]                       # 0x08: the all-ones code
_AC_VALID = set(AC_ALL)


def kraft_ok(bits):
    """sum(BITS[l] / 2**(l + 1)) <= 1, in integers; -> (holds, complete)."""
    assert len(bits) == 16 and all(0 <= b <= 255 for b in bits), bits
    s = sum(b << (15 - l) for l, b in enumerate(bits))
    return s <= 1 << 16, s == 1 << 16


def _checked(bits, vals, complete=None):
    ok, full = kraft_ok(bits)
    assert ok, ('over-subscribed', bits)
    assert complete is None or full == complete, (bits, complete)
    assert sum(bits) == len(vals) == len(set(vals)) and all(0 <= v <= 255 for v in vals)
    return list(bits), list(vals)


def ladder8(cls):
    return _checked([1] * 7 + [2] + [0] * 8, AC_L8 if cls else list(range(9)), True)


def ladder16(cls):
    """The +-1 symbols of long runs on the short codes, runs of 1 and 0 and EOB on the 15-bit
    and the two 16-bit codes (EOB the all-ones one); DC: five filler symbols on the short
    codes, the large categories last."""
    if cls:
        return _checked([1] * 15 + [2], [(r << 4) | 1 for r in range(15, 1, -1)] + [0x11, 0x01, 0x00], True)
    return _checked([1] * 15 + [2], [12, 13, 14, 15, 16] + list(range(12)), True)


AC_L16FF = [0x01, 0x11, 0x21, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0xF0, 0x31, 0x41, 0x00, 0x1A, 0x0A]


def ladder16ff(cls):
    """ladder16 with the all-ones 16-bit code on symbol 0x0A (run 0, size 10): a 1023 is 26
    1-bits, a symbol that spans five data bytes, all of them 0xFF, at every bit offset.  DC as
    ladder16: category 11 on the all-ones code, so a difference of 2047 is 27 1-bits."""
    return _checked([1] * 15 + [2], AC_L16FF, True) if cls else ladder16(0)


GAP_BITS = [0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 2, 4]


def gap(cls):
    """Seven codes of 2..8 bits, ten of 13..16; the frequent symbols spread over the long
    lengths.  The code after a -1 on the first 13-bit code (0x01) is often the 2-bit code
    (0x11): the 16 bits then equal limit[] of the empty lengths exactly."""
    if cls:
        vals = [0x11, 0xF1, 0xE1, 0xD1, 0xC1, 0xB1, 0xA1] + [0x01, 0x41, 0x21, 0x51, 0x31, 0x61, 0x00, 0x71, 0x81, 0x91]
    else:
        vals = [0, 1, 12, 13, 14, 15, 16] + [11, 2, 10, 3, 9, 4, 8, 5, 6, 7]
    return _checked(GAP_BITS, vals, False)


FLAT8_BITS = [0] * 6 + [1, 253, 2] + [0] * 7


def flat8(cls):
    """All 256 byte values; AC: 0x01 and EOB on the two 9-bit codes, DC: categories 10 and 11."""
    tail = [0x01, 0x00] if cls else [10, 11]
    return _checked(FLAT8_BITS, [v for v in range(256) if v not in tail] + tail, True)


def random_table(cls, seed, complete=True):
    """A random code tree of depth <= 16 over baseline's symbols; incomplete: two leaves more,
    then the last (all-ones) code and one other dropped."""
    rng = np.random.default_rng(seed)
    syms = AC_ALL if cls else list(range(12))
    n = len(syms) + (0 if complete else 2)
    depth = [1, 1]
    while len(depth) < n:
        cand = [i for i, d in enumerate(depth) if d < 16]
        i = max(rng.choice(cand, 2), key=lambda j: depth[j])      # deeper leaves split more often
        d = depth.pop(int(i))
        depth += [d + 1, d + 1]
    depth.sort()
    if not complete:
        depth.pop()
        depth.pop(int(rng.integers(len(depth))))
    bits = [depth.count(l) for l in range(1, 17)]
    return _checked(bits, [int(v) for v in rng.permutation(syms)], complete)


FAMILIES = {'ladder8': ladder8, 'ladder16': ladder16, 'ladder16ff': ladder16ff, 'gap': gap, 'flat8': flat8,
            'random': lambda cls: random_table(cls, 101 + cls, True),
            'random_open': lambda cls: random_table(cls, 201 + cls, False)}
CROSSED = ((1, 0), (0, 1), (1, 1))


def family_huff(name):
    """The same family in all four slots (different symbol orders per class only)."""
    f = FAMILIES[name]
    return {(0, 0): f(0), (0, 1): f(0), (1, 0): f(1), (1, 1): f(1)}


def mixed_huff():
    """Four families in one file."""
    return {(0, 0): ladder8(0), (0, 1): flat8(0), (1, 0): ladder16(1), (1, 1): random_table(1, 77, False)}


# --------------------------------------------------------------------- streams --

def dc_half_range(table):
    """h: DC values in [-h, h] differ by at most 2**cmax - 1, cmax the largest category c with
    0..c all in the table."""
    vals, c = set(table[1]), 0
    assert 0 in vals
    while c + 1 in vals and c + 1 < 12:
        c += 1
    return min(1000, ((1 << c) - 1) // 2)


def ac_block(rng, syms, weight, eob, zrl=0.05, ones=0.0, top=255):
    """One zigzag block whose run/size symbols all come from syms.  ones: the chance that a
    step is the value `top` (255 on symbol 0x08, 1023 on 0x0A: all 1-bits on the all-ones code)."""
    zz = np.zeros(64, np.int64)
    nz = [(s >> 4, s & 15) for s in syms if s & 15]
    has_eob, has_zrl = 0x00 in syms, 0xF0 in syms
    k = 1
    while k < 64:
        if ones and rng.random() < ones:
            zz[k] = top
            k += 1
            continue
        if has_eob and rng.random() < eob:
            break
        skip = 16 if has_zrl and k + 16 <= 63 and rng.random() < zrl else 0
        cand = [(r, s) for r, s in nz if k + skip + r <= 63]
        if not cand:
            break
        p = np.array([weight(r, s) for r, s in cand], np.float64)
        r, s = cand[int(rng.choice(len(cand), p=p / p.sum()))]
        mag = int(rng.integers(1 << (s - 1), 1 << s))
        k += skip + r
        zz[k] = mag if rng.random() < 0.5 else -mag
        k += 1
    assert has_eob or k == 64
    return zz


def fill(rng, H, W, mode, huff, scan_tables, weight, eob=0.12, ones=None, top=255):
    """MCU-padded grids (padding blocks filled like the others) from the symbols of each
    component's tables.  ones: per block, one of these chances of a step of value `top`."""
    out = []
    for c, (pr, pc) in enumerate(ir.padded_shapes(H, W, mode)):
        td, ta = scan_tables[c]
        syms = [s for s in huff[(1, ta)][1] if s in _AC_VALID]
        assert not ones or je.category(top) in syms          # run 0, top's size
        h = dc_half_range(huff[(0, td)])
        b = np.zeros((pr, pc, 64), np.int64)
        for y in range(pr):
            for x in range(pc):
                zz = ac_block(rng, syms, weight, eob, ones=float(rng.choice(ones)) if ones else 0.0, top=top)
                zz[0] = rng.integers(-h, h + 1)
                b[y, x, je.ZIGZAG] = zz
        out.append(b)
    return out


def ff_dense(H, W, mode, interleaved=True, top=255, dc=(255, 0)):
    """Every AC coefficient `top`; a component's DC alternates dc[0] / dc[1] along its scan order."""
    shapes, (_, grids, _) = ir.padded_shapes(H, W, mode), ir.geometry(H, W, mode)
    out = [np.full(s + (64,), top, np.int64) for s in shapes]
    for p in out:
        p[:, :, 0] = dc[1]
    if interleaved:
        seen = [0, 0, 0]
        for c, y, x in ir.mcu_order(H, W, mode):
            out[c][y, x, 0] = dc[seen[c] & 1]
            seen[c] += 1
    else:
        for p, (gr, gc) in zip(out, grids):
            p[:gr, :gc, 0] = np.where(np.arange(gr * gc) & 1, dc[1], dc[0]).reshape(gr, gc)
    return out


def stream(name, rng, H, W, mode, huff, scan_tables, interleaved=True):
    if name == 'ff_dense':
        return ff_dense(H, W, mode, interleaved)
    if name == 'ff_dense10':     # 26 1-bits per coefficient; DC differences of +-2047
        return ff_dense(H, W, mode, interleaved, 1023, (1023, -1024))
    if name == 'ff_mixed10':
        return fill(rng, H, W, mode, huff, scan_tables, lambda r, s: 1.0, eob=0.03, ones=(0.0, 0.4, 0.7, 0.9, 1.0), top=1023)
    if name == 'ff_mixed':
        return fill(rng, H, W, mode, huff, scan_tables, lambda r, s: 1.0, eob=0.03, ones=(0.0, 0.4, 0.7, 0.9, 1.0))
    if name == 'long_codes':
        return fill(rng, H, W, mode, huff, scan_tables, lambda r, s: 0.6 ** r if s == 1 else 1e-9, eob=0.04)
    assert name == 'sparse_random'
    return fill(rng, H, W, mode, huff, scan_tables, lambda r, s: 0.75 ** r * 0.7 ** s, eob=0.15)


# --------------------------------------------------------------------- writers --

def write3(padded, H, W, mode, qt, tq=(0, 0, 0), huff=None, scan_tables=ir.STD_SCAN_TABLES, ri=0):
    """Three non-interleaved scans (Y, Cb, Cr) over the T.81 grids with the file's own tables;
    ri: restart interval in blocks (a non-interleaved scan's MCU is one block)."""
    huff = ir.STD_HUFF if huff is None else huff
    _, grids, _ = ir.geometry(H, W, mode)
    codes = {k: je.huffman_codes(t) for k, t in huff.items()}
    out = bytearray(ir.headers(H, W, mode, qt, tq, huff, ri))
    for c, ((gr, gc), (td, ta)) in enumerate(zip(grids, scan_tables)):
        out += b'\xff\xda\x00\x08\x01' + bytes([c + 1, td << 4 | ta, 0, 63, 0])
        zz = np.asarray(padded[c], np.int64)[:gr, :gc].reshape(-1, 64)[:, je.ZIGZAG]
        per = ri if ri else len(zz)
        for i, a in enumerate(range(0, len(zz), per)):
            if i:
                out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
            w, pred = je.BitWriter(), 0
            for b in zz[a:a + per]:
                for cls, sym, mag, mlen in je.block_symbols(b, pred):
                    code, length = codes[(0, td) if cls == 'dc' else (1, ta)][sym]
                    w.put(code, length)
                    w.put(mag, mlen)
                pred = int(b[0])
            out += w.flush()
    return bytes(out + b'\xff\xd9')


def shift(data, k):
    """A COM segment with k payload bytes after SOI: the scan starts 4 + k bytes later."""
    assert data[:2] == b'\xff\xd8' and 0 <= k <= 3
    return data[:2] + b'\xff\xfe' + (2 + k).to_bytes(2, 'big') + b'jds'[:k] + data[2:]


def scans(data):
    """[(offset, entropy-coded bytes, RSTm included)] of a file's scans, found by walking its
    segments (the Python side's own parser, for the coverage assertions)."""
    p, out = 2, []
    while data[p + 1] != 0xD9:
        assert data[p] == 0xFF
        m, ln = data[p + 1], int.from_bytes(data[p + 2:p + 4], 'big')
        p += 2 + ln
        if m == 0xDA:
            e = p
            while not (data[e] == 0xFF and data[e + 1] != 0x00 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            out.append((p, data[p:e]))
            p = e
    return out


def intervals(seg):
    """A scan's stuffed bytes cut at its RSTm markers."""
    return ir._split_intervals(seg)


def ff_window_histogram(seg):
    """h[c]: windows of five consecutive data bytes (stuffing removed; per restart interval)
    that hold c bytes 0xFF."""
    h = np.zeros(6, np.int64)
    for part in intervals(seg):
        f = (np.frombuffer(part.replace(b'\xff\x00', b'\xff'), np.uint8) == 0xFF).astype(np.int64)
        if f.size >= 5:
            h += np.bincount(np.convolve(f, np.ones(5, np.int64), 'valid'), minlength=6)
    return h


def il_entries(padded, H, W, mode, scan_tables):
    """[((class, id), symbol, magnitude, magnitude bits)] of the interleaved scan, no restarts."""
    zz = [np.asarray(p, np.int64)[:, :, je.ZIGZAG] for p in padded]
    out, pred = [], [0, 0, 0]
    for c, y, x in ir.mcu_order(H, W, mode):
        td, ta = scan_tables[c]
        for cls, sym, mag, mlen in je.block_symbols(zz[c][y, x], pred[c]):
            out.append(((0, td) if cls == 'dc' else (1, ta), sym, mag, mlen))
        pred[c] = int(zz[c][y, x][0])
    return out


def pack(entries, huff):
    """je.BitWriter over il_entries' list; ('raw', bits, n, 0) puts n bits as they are."""
    codes = {k: je.huffman_codes(t) for k, t in huff.items()}
    w = je.BitWriter()
    for key, sym, mag, mlen in entries:
        if key == 'raw':
            w.put(sym, mag)
        else:
            w.put(*codes[key][sym])
            w.put(mag, mlen)
    return w.flush()


def code_lengths_used(entries, huff):
    """{(class, id): lengths of the codes the stream uses}."""
    codes = {k: je.huffman_codes(t) for k, t in huff.items()}
    out = {k: set() for k in huff}
    for key, sym, _, _ in entries:
        out[key].add(codes[key][sym][1])
    return out


# ----------------------------------------------------------------------- cases --

@functools.lru_cache(maxsize=None)
def case(family, strm, H, W, mode, seed=1, ri=0, interleaved=True, crossed=False, one_qt=False):
    """-> (file, written coefficients (planar, cropped), padded grids, huff, scan_tables).
    family 'mixed': four families in one file; crossed: the components use the table ids
    crosswise."""
    huff = mixed_huff() if family == 'mixed' else family_huff(family)
    st = CROSSED if crossed else ir.STD_SCAN_TABLES
    rng = np.random.default_rng([seed, H, W, MODES.index(mode)])
    padded = stream(strm, rng, H, W, mode, huff, st, interleaved)
    qt, tq = ({0: Q50}, (0, 0, 0)) if one_qt else ({0: Q50, 1: QC}, (0, 1, 1))
    data = (ir.write if interleaved else write3)(padded, H, W, mode, qt, tq, huff, st, ri)
    return data, ir.crop(padded, ir.geometry(H, W, mode)[1]), padded, huff, st


def defective_files():
    """{kind: file}: ordinary bounded decodes of bad data, built with je.BitWriter.
    'size12': a flat8 AC table whose stream really holds symbol 0x0C (size 12, outside
    baseline) with twelve magnitude bits; 'all_ones': gap's AC table (incomplete) with sixteen
    1-bits where a symbol belongs."""
    out = {}
    for kind, family, strm, repl in (('size12', 'flat8', 'sparse_random', ((1, 0), 0x0C, 0xABC, 12)),
                                     ('all_ones', 'gap', 'long_codes', ('raw', 0xFFFF, 16, 0))):
        H, W, mode = 24, 40, '4:2:0'
        _, _, padded, huff, st = case(family, strm, H, W, mode, seed=9)
        e = il_entries(padded, H, W, mode, st)
        assert pack(e, huff) == ir.entropy_segment(padded, H, W, mode, huff, st)
        ac = [i for i, (key, _, _, mlen) in enumerate(e) if key == (1, 0) and mlen]
        e[ac[len(ac) // 2]] = repl          # an AC symbol of a luma block, mid-scan
        out[kind] = ir.headers(H, W, mode, {0: Q50, 1: QC}, (0, 1, 1), huff) + ir.sos3(st) + pack(e, huff) + b'\xff\xd9'
    return out
