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
SOS header set to it).  The named double-defect cases are stored in full."""
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


class Lib:
    """The two parse calls of one libjds.so."""

    def __init__(self, path=None):
        from jds import _abi
        path = path or os.environ.get('JDS_LIB_PATH') or _abi.LIB_PATH
        self.path = path
        self.lib = C.CDLL(path)
        self.lib.jds_last_error.restype = C.c_char_p
        self.info = {'jfif': _abi.JfifInfo(), 'jpeg': _abi.JpegInfo()}
        self.fn = {'jfif': self.lib.jds_jfif_parse, 'jpeg': self.lib.jds_jpeg_parse}
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


def group_lines(lib, parser, data, group):
    """The ordered lines of one mutation group of one source."""
    n, end = len(data), first_sos_end(data)
    buf = (C.c_uint8 * max(n, 1)).from_buffer_copy(data)
    if group == 'orig':
        return [lib.line(parser, buf, n)]
    if group == 'trunc':
        return [lib.line(parser, buf, k) for k in list(range(end + 1)) + list(range(end + 7, n, 7))]
    v = int(group, 16)
    out = []
    for i in range(2, end):
        old, buf[i] = buf[i], v
        out.append(lib.line(parser, buf, n))
        buf[i] = old
    return out


GROUPS = ('orig', 'trunc') + tuple('%02X' % v for v in VALUES)


def digest(lines):
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def record(lib):
    out = {'sources': {}, 'digests': {}, 'double_defects': {}}
    for name, data in sources().items():
        out['sources'][name] = hashlib.sha256(data).hexdigest()
        for parser in PARSERS:
            for g in GROUPS:
                out['digests']['%s|%s|%s' % (name, parser, g)] = digest(group_lines(lib, parser, data, g))
    for name, data in double_defects().items():
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        out['double_defects'][name] = {p: list(lib.answer(p, buf, len(data))) for p in PARSERS}
    return out


def differences(lib, pins):
    """[(key, what differs)] of this library against the recorded pins; covers every case."""
    got, diffs = record(lib), []
    for sect in ('sources', 'digests', 'double_defects'):
        if sorted(got[sect]) != sorted(pins[sect]):
            diffs.append((sect, 'the set of cases differs'))
        for k, v in got[sect].items():
            if pins[sect].get(k) != v:
                diffs.append((k, 'recorded %r, now %r' % (pins[sect].get(k), v)))
    return diffs


if __name__ == '__main__':
    lib = Lib()
    if '--check' in sys.argv:
        d = differences(lib, json.load(open(PINS)))
        for k, what in d[:20]:
            print(k, what)
        print('%s: %d differences over %d parses' % (lib.path, len(d), lib.parses))
        sys.exit(1 if d else 0)
    pins = record(lib)
    with open(PINS, 'w') as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%s: %d digests, %d double-defect cases, %d parses -> %s (%d bytes)' % (
        lib.path, len(pins['digests']), len(pins['double_defects']), lib.parses, PINS, os.path.getsize(PINS)))
