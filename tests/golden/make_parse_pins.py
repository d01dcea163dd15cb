"""Recorder of tests/golden/parse_pins.json: what jds_jfif_parse and jds_jpeg_parse answer on a
set of small files and on every header mutation and truncation of them.

The fixture pins the two parsers' behaviour (return code, message, struct bytes) across a
rewrite of the parser: it is recorded from a build of the commit BEFORE the rewrite and the
rewritten code is tested against it (tests/test_parse_pins_cpu.py).  This script builds and
checks out nothing; it talks to the library JDS_LIB_PATH names (default: the in-tree build)
through ctypes.

    JDS_LIB_PATH=<the older build>/libjds.so python tests/golden/make_parse_pins.py          # record
    python tests/golden/make_parse_pins.py --check                                           # compare

Per source, parser and mutation group one SHA-256 over the group's ordered lines
`rc \\t message \\t sha256(struct bytes)` is stored (message on failure only, struct hash on
success only).  Groups: 'orig'; 'trunc' (every length up to the end of the first SOS header,
every 7th after it); one per value of VALUES (every byte from offset 2 to the end of the first
SOS header set to it).  The named double-defect cases are stored in full.

--pjpeg: the same for jds_pjpeg_parse and tests/golden/pjpeg_parse_pins.json
(tests/test_pjpeg_parse_pins_cpu.py), recorded from the build before the progressive walk was
put on the baseline walk's pieces.  Its sources are pure-Python files (tests/progressive_ref.py's
writer); its mutated bytes are the header's and, where this parser's own logic lives, every byte
of the marker segments between the scans (DHT, DRI, SOS).

    JDS_LIB_PATH=<the older build>/libjds.so python tests/golden/make_parse_pins.py --pjpeg
    python tests/golden/make_parse_pins.py --pjpeg --check"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, 'jpeg-dsp-studio_amd'), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

PINS = os.path.join(HERE, 'parse_pins.json')
VALUES = (0x00, 0x01, 0x03, 0x05, 0x11, 0x22, 0x3F, 0xC0, 0xC2, 0xC4, 0xD0, 0xD9, 0xDA, 0xDB, 0xDD, 0xFF)
PARSERS = ('jfif', 'jpeg')
PJPEG_PINS = os.path.join(HERE, 'pjpeg_parse_pins.json')
MAX_SOURCE_BYTES = 4096


def _q50():
    from oracle import cpu_ref
    return cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50)


def _sparse(seed, nblocks):
    """Sparse random blocks (row-major coefficient order): small files, every symbol class."""
    rng = np.random.default_rng(seed)
    b = rng.integers(-20, 21, (nblocks, 64)) * (rng.random((nblocks, 64)) < 0.08)
    b[:, 0] = rng.integers(-60, 61, nblocks)
    return b.astype(np.int16)


def _own(h, w, mode, ri=0):
    import restart_ref as rr
    from oracle import jpeg_entropy as je
    ny, nc = rr.counts(h, w, mode)
    cf = _sparse(h * 1000 + w, ny + 2 * nc)
    if ri:
        return rr.encode_jfif_rst(cf, h, w, mode, _q50(), ri)[0]
    return je.encode_jfif(cf, h, w, mode, _q50(), ny, nc)[0]


def _t81_three_scans(h, w, mode, ri):
    """Three Ns = 1 scans over the T.81 grids (not this library's floor-sized chroma)."""
    import interleaved_ref as ir
    import restart_ref as rr
    from oracle import jpeg_entropy as je
    grids = ir.geometry(h, w, mode)[1]
    out = bytearray(ir.headers(h, w, mode, {0: _q50()}, (0, 0, 0), ir.STD_HUFF, ri))
    for comp, (gr, gc) in enumerate(grids, start=1):
        blocks = _sparse(comp * 77 + ri, gr * gc)
        seg = rr.encode_scan_rst(blocks, comp > 1, ri)[0] if ri else je.encode_scan(blocks, comp > 1)[0]
        out += je.sos(comp) + seg
    return bytes(out + b'\xff\xd9')


def sources():
    """{name: bytes}, in a fixed order."""
    import gray_ref
    import huffopt_ref as hr
    import restart_ref as rr
    out = {}
    gold = os.path.join(HERE, 'jpeg_interleaved')
    for f in sorted(os.listdir(gold)):
        if f.endswith('.jpg'):
            out['golden/' + f[:-4]] = open(os.path.join(gold, f), 'rb').read()
    out['own/64x96_420'] = _own(64, 96, '4:2:0')
    out['own/64x96_422'] = _own(64, 96, '4:2:2')
    out['own/33x47_444'] = _own(33, 47, '4:4:4')
    out['own/2x2_420'] = _own(2, 2, '4:2:0')
    out['own/40x56_420_ri7'] = _own(40, 56, '4:2:0', 7)
    ny, nc = rr.counts(32, 48, '4:2:0')
    out['own/32x48_420_opt'] = hr.encode_jfif_opt(_sparse(5, ny + 2 * nc).reshape(-1), 32, 48, '4:2:0', _q50())[0]
    out['gray/19x27'] = gray_ref.write(_sparse(9, 3 * 4), gray_ref.default_prefix(19, 27, _q50()), False)
    out['t81/17x23_420'] = _t81_three_scans(17, 23, '4:2:0', 0)
    out['t81/17x23_420_ri2'] = _t81_three_scans(17, 23, '4:2:0', 2)
    for name, data in out.items():
        assert len(data) < MAX_SOURCE_BYTES, (name, len(data))
    return out


def _segment(data, marker, nth=0):
    """Offset of the nth segment with this marker, walking the headers up to the first SOS."""
    p = 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        if data[p + 1] == marker:
            if nth == 0:
                return p
            nth -= 1
        if data[p + 1] == 0xDA:
            break
        p += 2 + int.from_bytes(data[p + 2:p + 4], 'big')
    raise KeyError(hex(marker))


def first_sos_end(data):
    p = _segment(data, 0xDA)
    return p + 2 + int.from_bytes(data[p + 2:p + 4], 'big')


def double_defects():
    """{name: bytes}: files with two defects in one segment (or a defect whose report depends
    on the order of the checks); each parser must keep naming the one it names today."""
    import restart_ref as rr
    from oracle import jpeg_entropy as je
    base = _own(64, 96, '4:2:0')
    sof, sos = _segment(base, 0xC0), _segment(base, 0xDA)
    out = {}

    def patched(at, new, src=base):
        d = bytearray(src)
        d[at:at + len(new)] = new
        return bytes(d)
    # SOS: payload is Ns, Cs, Td|Ta, Ss, Se, Ah|Al from sos + 4
    out['sos_bad_spectral_and_table_ids_2_2'] = patched(sos + 6, bytes([0x22, 1, 63, 0]))
    out['sof_tq_5_5_5'] = patched(sof + 12, b'\x05', patched(sof + 15, b'\x05', patched(sof + 18, b'\x05')))
    out['sof_tq_5_0_0'] = patched(sof + 12, b'\x05')
    out['fourth_sos_names_component_7'] = base[:-2] + b'\xff\xda\x00\x08\x01\x07\x00\x00\x3f\x00' + b'\x00\xff\xd9'
    out['ns3_with_a_wrong_length'] = base[:sos] + b'\xff\xda\x00\x0a\x03\x01\x00\x02\x11\x00\x3f\x00' + base[sos + 10:]
    gray = base[:sof] + b'\xff\xc0\x00\x0b\x08\x00\x40\x00\x60\x01\x01\x11\x00' + base[sof + 19:]
    gsos = _segment(gray, 0xDA)
    out['gray_sof_then_malformed_dqt'] = gray[:gsos] + b'\xff\xdb\x00\x04\x20\x00' + gray[gsos:]
    ri4 = _own(64, 96, '4:2:0', 4)
    rst = ri4.index(b'\xff\xd1', first_sos_end(ri4))
    out['dri_4_one_rst_removed'] = ri4[:rst] + ri4[rst + 2:]
    ny, nc = rr.counts(17, 23, '4:2:0')
    out['dri_4_own_style_17x23'] = rr.encode_jfif_rst(_sparse(3, ny + 2 * nc), 17, 23, '4:2:0', _q50(), 4)[0]
    dht = _segment(base, 0xC4)
    dht_seg = base[dht:dht + 2 + int.from_bytes(base[dht + 2:dht + 4], 'big')]
    second_sos = base.index(je.sos(2))
    out['dht_redefined_between_scans'] = base[:second_sos] + dht_seg + base[second_sos:]
    return out


def pjpeg_sources():
    """{name: bytes}, in a fixed order: the scan scripts over the two geometries, the 64-scan
    gray file, and a baseline file (it answers "not progressive")."""
    import interleaved_ref as il
    import pjpeg_cases as pc
    import progressive_ref as pr
    out = {}
    for H, W, mode in pc.SCRIPT_GEOS:
        geo = '%dx%d_%s/' % (H, W, mode.replace(':', ''))
        out[geo + 'pillow'] = pr.write(pc.padded(H, W, mode), H, W, mode, pc.QT, pr.pillow_script(mode))
        for name in ('ids_2_3', 'shared_tables', 'ri1', 'ri5', 'stops_at_al1', 'bands'):
            out[geo + name] = pc.script_file(H, W, mode, name)[0]
    H, W, mode = pc.SCRIPT_GEOS[0]
    out['gray/64_scans'] = _pjpeg_gray_scans(64)
    out['baseline/%dx%d' % (H, W)] = il.write(pc.padded(H, W, mode), H, W, mode, pc.QT)
    for name, data in out.items():
        assert len(data) < MAX_SOURCE_BYTES, (name, len(data))
    return out


def _pjpeg_gray_scans(n):
    """The gray file of test_refusals_by_name: one scan per coefficient; 65: DC in two passes."""
    import pjpeg_cases as pc
    import progressive_ref as pr
    H, W, mode = pc.SCRIPT_GEOS[0]
    g = [np.asarray(pc.padded(H, W, mode)[0])[:3, :5]]
    s = [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)]
    if n == 65:
        s = [((0,), 0, 0, 0, 1)] + s[1:] + [((0,), 0, 0, 1, 0)]
    return pr.write(g, H, W, 'gray', {0: pc.QT[0]}, s)


def pjpeg_double_defects():
    """{name: bytes}: progressive files whose report depends on the order of the checks."""
    import pjpeg_cases as pc
    import progressive_ref as pr
    H, W, mode = pc.SCRIPT_GEOS[0]
    good = pr.write(pc.padded(H, W, mode), H, W, mode, pc.QT, pr.pillow_script(mode))
    data0 = [a for a, _ in pc._scan_ranges(good)]        # each scan's first data byte; Ss, Se, Ah|Al end its SOS

    def patched(at, new, src=good):
        d = bytearray(src)
        d[at:at + len(new)] = new
        return bytes(d)
    out = {}
    out['sos_ss_above_se_and_al_14'] = patched(data0[1] - 3, bytes([6, 5, 0x0E]))
    out['ac_scan_ns3_names_an_undefined_table'] = patched(data0[0] - 8, b'\x33', patched(data0[0] - 3, bytes([1, 5])))
    out['refinement_before_first_pass_with_wrong_ah'] = patched(data0[1] - 1, b'\x31')
    s65 = _pjpeg_gray_scans(65)
    out['scan_65_also_malformed'] = patched(pc._scan_ranges(s65)[64][0] - 3, bytes([6, 5]), s65)
    dht = _segment(good, 0xC4)
    out['dht_bad_header_and_oversubscribed'] = patched(dht + 4, b'\x24\x03')
    sof = _segment(good, 0xC2)
    out['sof2_precision_12_and_4_components'] = patched(sof + 9, b'\x04', patched(sof + 4, b'\x0c'))
    return out


# What a fixture is made of: its file, its parsers, its inputs, and whether the segments
# between the scans are mutated too.
BASELINE = dict(pins=PINS, parsers=PARSERS, sources=sources, double_defects=double_defects, later=False)
PJPEG = dict(pins=PJPEG_PINS, parsers=('pjpeg',), sources=pjpeg_sources, double_defects=pjpeg_double_defects, later=True)


class Lib:
    """The parse calls of one libjds.so."""

    def __init__(self, path=None):
        from jds import _abi
        path = path or os.environ.get('JDS_LIB_PATH') or _abi.LIB_PATH
        self.path = path
        self.lib = C.CDLL(path)
        self.lib.jds_last_error.restype = C.c_char_p
        self.info = {'jfif': _abi.JfifInfo(), 'jpeg': _abi.JpegInfo()}
        self.fn = {'jfif': self.lib.jds_jfif_parse, 'jpeg': self.lib.jds_jpeg_parse}
        if hasattr(self.lib, 'jds_pjpeg_parse'):
            self.info['pjpeg'], self.fn['pjpeg'] = _abi.PjpegInfo(), self.lib.jds_pjpeg_parse
        for f in self.fn.values():
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        self.parses = 0

    def answer(self, parser, buf, n):
        """(rc, message) of one parse; the message is '' on success."""
        info = self.info[parser]
        rc = self.fn[parser](buf, n, C.byref(info))
        self.parses += 1
        return rc, ('' if rc == 0 else self.lib.jds_last_error().decode(errors='replace'))

    def line(self, parser, buf, n):
        rc, msg = self.answer(parser, buf, n)
        h = hashlib.sha256(bytes(self.info[parser])).hexdigest() if rc == 0 else ''
        return '%d\t%s\t%s' % (rc, msg, h)


def later_segments(lib, data):
    """The bytes of the marker segments between the scans, by this library's own parse of the
    file (the 'orig' group pins that parse, struct bytes and all)."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    if lib.answer('pjpeg', buf, len(data))[0] != 0:
        return []
    info = lib.info['pjpeg']
    sc = [info.scan[i] for i in range(info.n_scans)]
    return [i for a, b in zip(sc, sc[1:]) for i in range(a.offset + a.length, b.offset)]


def group_lines(lib, parser, data, group, later=False):
    """The ordered lines of one mutation group of one source."""
    n, end = len(data), first_sos_end(data)
    where = list(range(2, end)) + (later_segments(lib, data) if later and group not in ('orig', 'trunc') else [])
    buf = (C.c_uint8 * max(n, 1)).from_buffer_copy(data)
    if group == 'orig':
        return [lib.line(parser, buf, n)]
    if group == 'trunc':
        return [lib.line(parser, buf, k) for k in list(range(end + 1)) + list(range(end + 7, n, 7))]
    v = int(group, 16)
    out = []
    for i in where:
        old, buf[i] = buf[i], v
        out.append(lib.line(parser, buf, n))
        buf[i] = old
    return out


GROUPS = ('orig', 'trunc') + tuple('%02X' % v for v in VALUES)


def digest(lines):
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def record(lib, fx=BASELINE):
    out = {'sources': {}, 'digests': {}, 'double_defects': {}}
    for name, data in fx['sources']().items():
        out['sources'][name] = hashlib.sha256(data).hexdigest()
        for parser in fx['parsers']:
            for g in GROUPS:
                out['digests']['%s|%s|%s' % (name, parser, g)] = digest(group_lines(lib, parser, data, g, fx['later']))
    for name, data in fx['double_defects']().items():
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        out['double_defects'][name] = {p: list(lib.answer(p, buf, len(data))) for p in fx['parsers']}
    return out


def differences(lib, pins, fx=BASELINE):
    """[(key, what differs)] of this library against the recorded pins; covers every case."""
    got, diffs = record(lib, fx), []
    for sect in ('sources', 'digests', 'double_defects'):
        if sorted(got[sect]) != sorted(pins[sect]):
            diffs.append((sect, 'the set of cases differs'))
        for k, v in got[sect].items():
            if pins[sect].get(k) != v:
                diffs.append((k, 'recorded %r, now %r' % (pins[sect].get(k), v)))
    return diffs


if __name__ == '__main__':
    lib = Lib()
    fx = PJPEG if '--pjpeg' in sys.argv else BASELINE
    PINS = fx['pins']
    if '--check' in sys.argv:
        d = differences(lib, json.load(open(PINS)), fx)
        for k, what in d[:20]:
            print(k, what)
        print('%s: %d differences over %d parses' % (lib.path, len(d), lib.parses))
        sys.exit(1 if d else 0)
    pins = record(lib, fx)
    with open(PINS, 'w') as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%s: %d digests, %d double-defect cases, %d parses -> %s (%d bytes)' % (
        lib.path, len(pins['digests']), len(pins['double_defects']), lib.parses, PINS, os.path.getsize(PINS)))
