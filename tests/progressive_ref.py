"""Reference decoder and writer of progressive JPEGs (T.81 Annex G), in pure
Python from the standard's procedures and independent of the library's C++
core: what the progressive tests compare against.

    decode(data) -> dict
        walks the markers, keeps the Huffman tables in effect at every SOS and
        applies each scan to the coefficients: DC first (G.1.2.1), DC
        refinement, AC first with EOBRUN (G.1.2.2), AC refinement (G.1.2.3).
          'planar'   Y, Cb, Cr (or the one plane), each component's blocks in
                     raster order of its T.81 grid, row-major inside a block
                     (int16, flat): the layout of jds.entropy.decode_pjpeg
          'padded'   per component the MCU-padded grid (rows, cols, 64), row-major
          'scans'    [(components, ss, se, ah, al)] in file order
          'complete' every coefficient was coded down to Al = 0
          'H', 'W', 'mode' ('gray' for one component), 'grids', 'qt', 'tq', 'ri'
    write(padded, H, W, mode, qt, script, ri=0, tq=..., table_ids=..., shared_tables=False) -> bytes
        any scan script over MCU-padded grids (interleaved_ref.random_padded's
        form; mode 'gray': one grid): script = [(components, ss, se, ah, al)],
        components 0-based.  Huffman tables are built per scan from the scan's
        own symbol counts (T.81 K.2 / K.3 through huffopt_ref.optimal_table) and
        defined in a DHT in front of its SOS; shared_tables: one table set from
        the whole file's counts in front of the first SOS.  table_ids:
        {component: (dc id, ac id)}.  ri: DRI, in MCUs of each scan.
"""
import numpy as np

import huffopt_ref
import interleaved_ref as il
from oracle import jpeg_entropy as je

ZZ = je.ZIGZAG
DEFAULT_IDS = {0: (0, 0), 1: (1, 1), 2: (1, 1)}


def geometry(H, W, mode):
    if mode == 'gray':
        g = (-(-H // 8), -(-W // 8))
        return [(1, 1)], [g], g
    return il.geometry(H, W, mode)


def padded_shapes(H, W, mode):
    samp, _, mcu = geometry(H, W, mode)
    return [(mcu[0] * vs, mcu[1] * hs) for hs, vs in samp]


def scan_blocks(H, W, mode, comps):
    """[[(component, row, col), ..] per MCU] of a scan, in scan order."""
    samp, grids, mcu = geometry(H, W, mode)
    if len(comps) == 1:
        c = comps[0]
        gr, gc = grids[c]
        return [[(c, y, x)] for y in range(gr) for x in range(gc)]
    out = []
    for my in range(mcu[0]):
        for mx in range(mcu[1]):
            out.append([(c, my * samp[c][1] + by, mx * samp[c][0] + bx)
                        for c in comps for by in range(samp[c][1]) for bx in range(samp[c][0])])
    return out


# --- decoder ----------------------------------------------------------------

class _Reader(je.BitReader):
    def symbol(self, table):
        code, length = 0, 0
        while True:
            code = (code << 1) | self.bit()
            length += 1
            if (length, code) in table:
                return table[(length, code)]
            assert length < 16, 'bad Huffman code'


def _decode_scan(zz, H, W, mode, comps, tabs, ss, se, ah, al, seg, ri):
    """zz: per component (rows, cols, 64) in zigzag order, updated in place."""
    mcus = scan_blocks(H, W, mode, comps)
    per = ri if ri else len(mcus)
    parts = il._split_intervals(seg) if ri else [seg]
    assert len(parts) == -(-len(mcus) // per), 'restart markers do not match the interval'
    p1 = 1 << al
    for i, part in enumerate(parts):
        r, pred, eobrun = _Reader(part), {c: 0 for c in comps}, 0
        for mcu in mcus[i * per:(i + 1) * per]:
            for c, y, x in mcu:
                b = zz[c][y, x]
                if ss == 0:
                    if ah == 0:
                        s = r.symbol(tabs[(0, c)])
                        pred[c] += je._extend(r.bits(s), s)
                        b[0] = pred[c] * p1
                    elif r.bit():
                        b[0] |= p1
                elif ah == 0:
                    if eobrun:
                        eobrun -= 1
                        continue
                    k = ss
                    while k <= se:
                        rs = r.symbol(tabs[(1, c)])
                        run, s = rs >> 4, rs & 15
                        if s == 0:
                            if run < 15:
                                eobrun = (1 << run) + r.bits(run) - 1
                                break
                            k += 16
                            continue
                        k += run
                        assert k <= se, 'run past Se'
                        b[k] = je._extend(r.bits(s), s) * p1
                        k += 1
                else:
                    k = ss
                    if eobrun == 0:
                        while k <= se:
                            rs = r.symbol(tabs[(1, c)])
                            run, s = rs >> 4, rs & 15
                            new = 0
                            if s:
                                assert s == 1, 'refinement symbol with size > 1'
                                new = p1 if r.bit() else -p1
                            elif run < 15:
                                eobrun = (1 << run) + r.bits(run)
                                break
                            while True:       # pass `run` coefficients without history (ZRL: 16)
                                assert k <= se, 'run past Se'
                                if b[k]:
                                    if r.bit():
                                        b[k] += p1 if b[k] > 0 else -p1
                                else:
                                    run -= 1
                                    if run < 0:
                                        break
                                k += 1
                            if s:
                                b[k] = new
                            k += 1
                    if eobrun:
                        while k <= se:
                            if b[k] and r.bit():
                                b[k] += p1 if b[k] > 0 else -p1
                            k += 1
                        eobrun -= 1
        assert eobrun == 0, 'EOBRUN beyond the interval'
        assert r.p == len(part), 'interval holds more bytes than its blocks'


def decode(data):
    data = bytes(data)
    assert data[:2] == b'\xff\xd8'
    p, qt, huff, ri, scans = 2, {}, {}, 0, []
    H = W = mode = tq = None
    zz = None
    last_al = None
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
                t[ZZ] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[seg[q] & 15] = t.reshape(8, 8)
                q += 65
        elif m == 0xC2:
            assert seg[0] == 8 and seg[5] in (1, 3)
            H, W = int.from_bytes(seg[1:3], 'big'), int.from_bytes(seg[3:5], 'big')
            if seg[5] == 1:
                mode, tq = 'gray', [seg[8]]
            else:
                assert [seg[6], seg[9], seg[12]] == [1, 2, 3] and seg[10] == 0x11 and seg[13] == 0x11
                mode, tq = il.MODES[seg[7]], [seg[8], seg[11], seg[14]]
            gray_id = seg[6]
            zz = [np.zeros(s + (64,), np.int64) for s in padded_shapes(H, W, mode)]
            last_al = [[None] * 64 for _ in zz]
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
            comps = [0 if mode == 'gray' and seg[1 + 2 * i] == gray_id else seg[1 + 2 * i] - 1 for i in range(ns)]
            ss, se, a = seg[1 + 2 * ns:4 + 2 * ns]
            ah, al = a >> 4, a & 15
            tabs = {}
            for i, c in enumerate(comps):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                for cls, th in ((0, td), (1, ta)):
                    if (cls, th) in huff and ((cls == 0) == (ss == 0)):
                        tabs[(cls, c)] = {(l, cd): s for s, (cd, l) in je.huffman_codes(huff[(cls, th)]).items()}
                for k in range(ss, se + 1):
                    assert last_al[c][k] == (ah if ah else None), 'inconsistent progression'
                    last_al[c][k] = al
            e = p
            while not (data[e] == 0xFF and data[e + 1] != 0x00 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            _decode_scan(zz, H, W, mode, comps, tabs, ss, se, ah, al, data[p:e], ri)
            scans.append((comps, ss, se, ah, al))
            p = e
    _, grids, mcu = geometry(H, W, mode)
    padded = []
    for z in zz:
        nat = np.zeros_like(z)
        nat[:, :, ZZ] = z
        padded.append(nat)
    return {'H': H, 'W': W, 'mode': mode, 'qt': qt, 'tq': tq, 'qtables': np.stack([qt[t] for t in tq]), 'ri': ri,
            'grids': grids, 'mcu': mcu, 'scans': scans, 'padded': padded, 'planar': il.crop(padded, grids),
            'complete': all(v == 0 for la in last_al for v in la)}


# --- writer -----------------------------------------------------------------

def _mag(v, s):
    """The s magnitude bits of v (T.81 F.1.2.1: negative values as v - 1)."""
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


class _Tokens:
    """One scan's output before its tables exist: ('s', key, symbol), ('b', value, nbits), ('r', m)."""

    def __init__(self):
        self.t = []

    def sym(self, key, s):
        self.t.append(('s', key, s))

    def bits(self, v, n):
        if n:
            self.t.append(('b', v, n))


def _scan_tokens(zz, H, W, mode, comps, keys, ss, se, ah, al, ri):
    """keys[c]: the table key (class, id) the scan's symbols of component c are coded with."""
    out = _Tokens()
    mcus = scan_blocks(H, W, mode, comps)
    per = ri if ri else len(mcus)
    state = {'eobrun': 0, 'be': []}

    def flush_eobrun(key):
        if state['eobrun']:
            n = state['eobrun'].bit_length() - 1
            out.sym(key, n << 4)
            out.bits(state['eobrun'] - (1 << n), n)
            state['eobrun'] = 0
        for b in state['be']:
            out.bits(b, 1)
        state['be'] = []

    # (blocks whose band is empty at this Al only lengthen the end-of-band run: found at once)
    empty = {c: ~((np.abs(zz[c][:, :, ss:se + 1]) >> al).any(axis=2)) for c in comps} if ss else None
    for i, a in enumerate(range(0, len(mcus), per)):
        if i:
            out.t.append(('r', (i - 1) & 7))
        pred = {c: 0 for c in comps}
        for mcu in mcus[a:a + per]:
            for c, y, x in mcu:
                key = keys[c]
                if ss and empty[c][y, x]:
                    state['eobrun'] += 1
                    if state['eobrun'] == 0x7FFF:
                        flush_eobrun(key)
                    continue
                b = [int(v) for v in zz[c][y, x]]
                if ss == 0:
                    v = b[0] >> al                      # DC: an arithmetic shift (G.1.2.1)
                    if ah == 0:
                        d = v - pred[c]
                        pred[c] = v
                        s = je.category(d)
                        out.sym(key, s)
                        out.bits(_mag(d, s), s)
                    else:
                        out.bits(v & 1, 1)
                    continue
                ab = [abs(v) >> al for v in b]          # AC: division, rounding toward zero
                if ah == 0:
                    run = 0
                    for k in range(ss, se + 1):
                        if ab[k] == 0:
                            run += 1
                            continue
                        flush_eobrun(key)
                        while run > 15:
                            out.sym(key, 0xF0)
                            run -= 16
                        s = ab[k].bit_length()
                        out.sym(key, run << 4 | s)
                        out.bits(_mag(ab[k] if b[k] > 0 else -ab[k], s), s)
                        run = 0
                    if run:
                        state['eobrun'] += 1
                        if state['eobrun'] == 0x7FFF:
                            flush_eobrun(key)
                else:
                    new = [k for k in range(ss, se + 1) if ab[k] == 1]
                    eob = new[-1] if new else -1
                    run, br = 0, []
                    for k in range(ss, se + 1):
                        if ab[k] == 0:
                            run += 1
                            continue
                        while run > 15 and k <= eob:
                            flush_eobrun(key)
                            out.sym(key, 0xF0)
                            run -= 16
                            for v in br:
                                out.bits(v, 1)
                            br = []
                        if ab[k] > 1:
                            br.append(ab[k] & 1)
                            continue
                        flush_eobrun(key)
                        out.sym(key, run << 4 | 1)
                        out.bits(1 if b[k] > 0 else 0, 1)
                        for v in br:
                            out.bits(v, 1)
                        br, run = [], 0
                    if run or br:
                        state['eobrun'] += 1
                        state['be'] += br
                        if state['eobrun'] == 0x7FFF:
                            flush_eobrun(key)
        if ss:
            flush_eobrun(keys[comps[0]])
    return out.t


def _emit(tokens, codes):
    out, w = bytearray(), je.BitWriter()
    for t in tokens:
        if t[0] == 's':
            code, length = codes[t[1]][t[2]]
            w.put(code, length)
        elif t[0] == 'b':
            w.put(t[1], t[2])
        else:
            out += w.flush() + bytes([0xFF, 0xD0 + t[1]])
            w = je.BitWriter()
    return bytes(out + w.flush())


def _table(tokens, key):
    freq = np.zeros(256, np.int64)
    for t in tokens:
        if t[0] == 's' and t[1] == key:
            freq[t[2]] += 1
    bits, vals, fell = huffopt_ref.optimal_table(freq)
    assert not fell
    return bits, vals


def frame_header(H, W, mode, qt, tq, app0=False):
    out = bytearray(b'\xff\xd8')
    if app0:
        out += b'\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
    for i in sorted(qt):
        q = np.asarray(qt[i], np.float64).reshape(64)[ZZ]
        out += b'\xff\xdb\x00\x43' + bytes([i]) + bytes(int(v) for v in q)
    nf = 1 if mode == 'gray' else 3
    out += b'\xff\xc2' + (8 + 3 * nf).to_bytes(2, 'big') + b'\x08' + int(H).to_bytes(2, 'big') + int(W).to_bytes(2, 'big')
    if nf == 1:
        out += bytes([1, 1, 0x11, tq[0]])
    else:
        out += bytes([3, 1, je.SAMPLING[mode], tq[0], 2, 0x11, tq[1], 3, 0x11, tq[2]])
    return bytes(out)


def sos(comps, ids, ss, se, ah, al):
    return b'\xff\xda' + (6 + 2 * len(comps)).to_bytes(2, 'big') + bytes([len(comps)]) \
        + bytes(sum(([c + 1, ids[c][0] << 4 | ids[c][1]] for c in comps), [])) + bytes([ss, se, ah << 4 | al])


def write(padded, H, W, mode, qt, script, ri=0, tq=None, table_ids=None, shared_tables=False, tamper=None):
    """tamper(scan index, keys, tokens) -> tokens: edits a scan's symbol stream before its tables
    are built (the hostile files of the tests: defects by construction)."""
    ids = dict(DEFAULT_IDS if table_ids is None else table_ids)
    tq = ([0] if mode == 'gray' else [0, 1, 1]) if tq is None else list(tq)
    shapes = padded_shapes(H, W, mode)
    assert [tuple(np.asarray(p).shape[:2]) for p in padded] == shapes, ([np.asarray(p).shape for p in padded], shapes)
    zz = [np.asarray(p, np.int64).reshape(s + (64,))[:, :, ZZ] for p, s in zip(padded, shapes)]
    toks = []
    for comps, ss, se, ah, al in script:
        keys = {c: (0 if ss == 0 else 1, ids[c][0 if ss == 0 else 1]) for c in comps}
        tk = _scan_tokens(zz, H, W, mode, list(comps), keys, ss, se, ah, al, ri)
        toks.append((keys, tamper(len(toks), keys, tk) if tamper else tk))
    out = bytearray(frame_header(H, W, mode, qt, tq))
    if ri:
        out += b'\xff\xdd\x00\x04' + int(ri).to_bytes(2, 'big')
    shared = {}
    if shared_tables:
        every = [t for _, tk in toks for t in tk]
        for key in sorted({k for keys, _ in toks for k in keys.values()}):
            if any(t[0] == 's' and t[1] == key for t in every):
                shared[key] = _table(every, key)
                out += huffopt_ref.dht(key[0] << 4 | key[1], *shared[key])
    for (comps, ss, se, ah, al), (keys, tk) in zip(script, toks):
        codes = {}
        for key in sorted(set(keys.values())):
            if not any(t[0] == 's' and t[1] == key for t in tk):
                continue                                   # (a DC refinement scan reads no table)
            tab = shared[key] if shared_tables else _table(tk, key)
            if not shared_tables:
                out += huffopt_ref.dht(key[0] << 4 | key[1], *tab)
            codes[key] = je.huffman_codes(tab)
        out += sos(list(comps), ids, ss, se, ah, al) + _emit(tk, codes)
    return bytes(out + b'\xff\xd9')


# --- scripts ----------------------------------------------------------------

def pillow_script(mode):
    """The scan script libjpeg's jpeg_simple_progression gives (what Pillow writes)."""
    if mode == 'gray':
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
                ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
            ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def _each(mode, f):
    return [s for c in range(1 if mode == 'gray' else 3) for s in f(c)]


def scripts(mode):
    """{name: script}: the scan scripts Pillow never writes."""
    allc = (0,) if mode == 'gray' else (0, 1, 2)
    return {
        'full_spectrum': [(allc, 0, 0, 0, 0)] + _each(mode, lambda c: [((c,), 1, 63, 0, 0)]),
        'dc_per_component': _each(mode, lambda c: [((c,), 0, 0, 0, 0)]) + _each(mode, lambda c: [((c,), 1, 63, 0, 0)]),
        'al3_three_refinements': [(allc, 0, 0, 0, 3)] + _each(mode, lambda c: [((c,), 1, 63, 0, 3)])
        + [s for a in (2, 1, 0) for s in [(allc, 0, 0, a + 1, a)] + _each(mode, lambda c: [((c,), 1, 63, a + 1, a)])],
        'bands': [(allc, 0, 0, 0, 0)] + _each(mode, lambda c: [((c,), 1, 1, 0, 0), ((c,), 2, 2, 0, 0), ((c,), 3, 9, 0, 0),
                                                               ((c,), 10, 63, 0, 0)]),
        'stops_at_al1': [(allc, 0, 0, 0, 1)] + _each(mode, lambda c: [((c,), 1, 63, 0, 1)]),
    }
