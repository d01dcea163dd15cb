"""Baseline JPEG entropy coding on the GPU (include/jds.h: jds_encode_jfif,
jds_plan_entropy): the reference's quantised coefficients -> a standard JFIF
file (the reference itself only estimates the size,
utils/metrics.py:51-92).  Byte-for-byte definition: oracle/jpeg_entropy.py.
And back (jds_jfif_parse, jds_decode_jfif, jds_plan_entropy_decode): a
baseline file of that profile -> the coefficients, by a self-synchronising
parallel Huffman decode (DESIGN.md "Entropy decode").  Both directions take
restart intervals (DESIGN.md "Restart intervals"): the writer at the interval
restart_info() reports, the decoder at any, one lane per interval in one pass."""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _abi
from ._abi import check, lib, make_params


def restart_info() -> Tuple[int, int]:
    """(the restart interval the writer supports besides 0, the largest interval the decoder
    gives to one lane), in blocks."""
    w, m = C.c_int32(0), C.c_int32(0)
    check(lib().jds_entropy_restart_info(C.byref(w), C.byref(m)))
    return int(w.value), int(m.value)


def encode_jfif(coeffs: np.ndarray, H: int, W: int, mode: str, qtable: np.ndarray,
                device: int = 0, restart_interval: int = 0, optimize: bool = False) -> Tuple[bytes, List[int]]:
    """One frame: all_quantized_coeffs (int16, Y/Cb/Cr blocks) -> (file bytes,
    entropy-coded bits of the Y, Cb, Cr scans).  restart_interval: 0, or restart_info()[0]
    for a file with DRI and RSTm markers (every interval an independent stream).  optimize:
    the frame's own Huffman tables instead of the Annex K ones (jds_encode_jfif_opt,
    DESIGN.md "Optimised tables")."""
    p = make_params(50, qtable, mode, False, np.zeros(3))
    geo = _abi.geometry(p, H, W)
    cf = np.ascontiguousarray(coeffs, dtype=np.int16).reshape(-1)
    if cf.size != geo.coeffs_per_frame:
        raise ValueError(f'expected {geo.coeffs_per_frame} coefficients for {H}x{W} {mode}, got {cf.size}')
    n = C.c_int64(0)
    bits = (C.c_uint64 * 3)()
    # a random frame at high quality stays far below this; the C side reports the exact need
    cap = max(1 << 16, 8 * cf.size)
    while True:
        out = np.empty(cap, np.uint8)
        with _abi.lease(device) as ctx:
            if optimize:
                rc = lib().jds_encode_jfif_opt(ctx.handle, C.byref(p), H, W, int(restart_interval), cf.ctypes.data,
                                               out.ctypes.data, cap, C.byref(n), bits)
            elif restart_interval:
                rc = lib().jds_encode_jfif_rst(ctx.handle, C.byref(p), H, W, int(restart_interval), cf.ctypes.data,
                                               out.ctypes.data, cap, C.byref(n), bits)
            else:
                rc = lib().jds_encode_jfif(ctx.handle, C.byref(p), H, W, cf.ctypes.data, out.ctypes.data,
                                           cap, C.byref(n), bits)
        if rc == _abi.JDS_EINVAL and n.value > cap:
            cap = n.value
            continue
        check(rc)
        return out[:n.value].tobytes(), [int(b) for b in bits]


_MODE_NAMES = {v: k for k, v in _abi.JPEG_MODE_CODES.items()}


def _bytes_arg(data):
    """(keep-alive array, pointer, length) of a bytes-like file."""
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    if a.size == 0:
        raise ValueError('empty file')
    return a, a.ctypes.data, int(a.size)


def _info_dict(info: _abi.JfifInfo) -> dict:
    names = ('dc0', 'dc1', 'ac0', 'ac1')
    huff = {}
    for i, nm in enumerate(names):
        h = info.huff[i]
        if h.defined:
            huff[nm] = (list(h.bits), list(h.vals)[:h.n_vals])
    return {'H': int(info.H), 'W': int(info.W), 'mode': _MODE_NAMES[info.subsampling],
            'qtable': np.ctypeslib.as_array(info.qtable).astype(np.float64).reshape(8, 8),
            'scans': [{'component': int(s.component), 'dc_table': int(s.dc_table), 'ac_table': int(s.ac_table),
                       'restart_interval': int(s.restart_interval), 'offset': int(s.offset),
                       'length': int(s.length)} for s in info.scan[:info.n_scans]],
            'huffman': huff, 'y_blocks': int(info.y_blocks), 'c_blocks': int(info.c_blocks),
            'coeffs_needed': int(info.coeffs_needed)}


def parse_jfif(data) -> dict:
    """jds_jfif_parse (host only, no GPU): geometry, table, scans and Huffman tables of a
    baseline JFIF of the profile this library writes.  ValueError for anything else."""
    a, p, n = _bytes_arg(data)
    info = _abi.JfifInfo()
    check(lib().jds_jfif_parse(p, n, C.byref(info)))
    return _info_dict(info)


def decode_info() -> Tuple[int, int]:
    """(bits per subsequence, subsequences per workgroup) of the GPU decoder."""
    s, g = C.c_int32(0), C.c_int32(0)
    check(lib().jds_entropy_decode_info(C.byref(s), C.byref(g)))
    return int(s.value), int(g.value)


def decode_jfif(data, device: int = 0) -> dict:
    """One file -> {'coeffs' (int16, reference layout), 'H', 'W', 'mode', 'qtable', 'rounds'}."""
    a, p, n = _bytes_arg(data)
    info = _abi.JfifInfo()
    check(lib().jds_jfif_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.coeffs_needed), np.int16)
    with _abi.lease(device) as ctx:
        check(lib().jds_decode_jfif(ctx.handle, p, n, cf.ctypes.data, cf.size, C.byref(info)))
    d = _info_dict(info)
    return {'coeffs': cf, 'H': d['H'], 'W': d['W'], 'mode': d['mode'], 'qtable': d['qtable'],
            'rounds': int(info.rounds)}


def host_decode_jfif(data, subseq_bits: int = 1024):
    """Test aid (jds_selftest_huffdec): the decoder's algorithm on the host with the
    kernels' shared core -> (coeffs, [rounds of the Y, Cb, Cr scans]).  No GPU."""
    a, p, n = _bytes_arg(data)
    info = _abi.JfifInfo()
    check(lib().jds_jfif_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.coeffs_needed), np.int16)
    rounds = (C.c_int32 * 3)()
    check(lib().jds_selftest_huffdec(p, n, int(subseq_bits), cf.ctypes.data, cf.size, rounds))
    return cf, [int(r) for r in rounds]


def optimal_table(freq):
    """Test aid (jds_selftest_huffopt, no GPU): the optimised table of freq[0..255] by the
    host/device core of k_ent_opt_tables -> (BITS[1..16], HUFFVAL, fell_back)."""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    if f.shape != (256,):
        raise ValueError('freq: 256 counts')
    bits, vals = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    n, fell = C.c_int32(0), C.c_int32(0)
    check(lib().jds_selftest_huffopt(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, C.byref(n), C.byref(fell)))
    return [int(b) for b in bits], [int(v) for v in vals[:n.value]], bool(fell.value)


def optimal_tables_dev(freqs, device: int = 0):
    """Test aid (jds_selftest_huffopt_dev): k_ent_opt_tables on n histograms (n x 256 counts)
    -> [(BITS, HUFFVAL, fell_back)]."""
    f = np.ascontiguousarray(freqs, dtype=np.uint32)
    if f.ndim != 2 or f.shape[1] != 256 or not len(f):
        raise ValueError('freqs: n x 256 counts')
    m = len(f)
    bits, vals = np.zeros((m, 16), np.uint8), np.zeros((m, 256), np.uint8)
    n, fell = np.zeros(m, np.int32), np.zeros(m, np.int32)
    with _abi.lease(device) as ctx:
        check(lib().jds_selftest_huffopt_dev(ctx.handle, f.ctypes.data, m, bits.ctypes.data, vals.ctypes.data,
                                             n.ctypes.data, fell.ctypes.data))
    return [([int(b) for b in bits[i]], [int(v) for v in vals[i, :n[i]]], bool(fell[i])) for i in range(m)]


def _jpeg_dict(info: _abi.JpegInfo) -> dict:
    names = ('dc0', 'dc1', 'ac0', 'ac1')
    huff = {nm: (list(info.huff[i].bits), list(info.huff[i].vals)[:info.huff[i].n_vals])
            for i, nm in enumerate(names) if info.huff[i].defined}
    scans = []
    for s in info.scan[:info.n_scans]:
        n = int(s.n_components)
        scans.append({'components': list(s.component)[:n], 'dc_tables': list(s.dc_table)[:n],
                      'ac_tables': list(s.ac_table)[:n], 'restart_interval': int(s.restart_interval),
                      'offset': int(s.offset), 'length': int(s.length)})
    return {'H': int(info.H), 'W': int(info.W), 'mode': _MODE_NAMES[info.subsampling],
            'components': 1 if info.subsampling == _abi.SS_GRAY else 3,
            'interleaved': bool(info.interleaved), 'reference_grid': bool(info.reference_grid),
            'single_table': bool(info.single_table),
            'qtables': np.ctypeslib.as_array(info.qtable).astype(np.float64).reshape(3, 8, 8),
            'tq': list(info.tq), 'sampling': [(int(info.hs[c]), int(info.vs[c])) for c in range(3)],
            'grids': [(int(info.grid_rows[c]), int(info.grid_cols[c])) for c in range(3)],
            'mcu': {'rows': int(info.mcu_rows), 'cols': int(info.mcu_cols), 'blocks': int(info.blocks_per_mcu)},
            'scans': scans, 'huffman': huff, 'coeffs_needed': int(info.coeffs_needed)}


def parse_jpeg(data) -> dict:
    """jds_jpeg_parse (host only, no GPU): a baseline JPEG with one interleaved scan or three
    non-interleaved ones, up to three quantisation tables, T.81 block grids; or a grayscale
    file ('mode': 'gray', 'components': 1: one scan of one component, whose sampling byte is
    ignored; 'qtables' and 'grids' keep three entries, zero for the absent components).  'grids': (rows,
    columns) of each component's block grid; 'mcu': the MCU grid and the blocks of an
    interleaved MCU; 'reference_grid': the grids are the ones parse_jfif accepts.  ValueError
    naming the feature for anything else."""
    a, p, n = _bytes_arg(data)
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_parse(p, n, C.byref(info)))
    return _jpeg_dict(info)


def decode_jpeg(data, device: int = 0) -> dict:
    """One file -> parse_jpeg's dict plus 'coeffs' (int16: Y, Cb, Cr planar, each component's
    blocks in raster order of its T.81 grid) and 'rounds'."""
    a, p, n = _bytes_arg(data)
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.coeffs_needed), np.int16)
    with _abi.lease(device) as ctx:
        check(lib().jds_decode_jpeg(ctx.handle, p, n, cf.ctypes.data, cf.size, C.byref(info)))
    d = _jpeg_dict(info)
    d['coeffs'] = cf
    d['rounds'] = int(info.rounds)
    return d


def host_decode_jpeg(data, subseq_bits: int = 1024):
    """Test aid (jds_selftest_jpegdec): decode_jpeg's algorithm on the host with the kernels'
    shared core -> (coeffs, [rounds per scan in file order]).  No GPU."""
    a, p, n = _bytes_arg(data)
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.coeffs_needed), np.int16)
    rounds = (C.c_int32 * 3)()
    check(lib().jds_selftest_jpegdec(p, n, int(subseq_bits), cf.ctypes.data, cf.size, rounds))
    return cf, [int(r) for r in rounds][:int(info.n_scans)]


def _pjpeg_dict(info: _abi.PjpegInfo) -> dict:
    """The frame in parse_jpeg's terms (as the baseline file of the same frame parses, without
    'scans' and 'huffman' entries of its own) plus the scan script."""
    d = _jpeg_dict(info.frame)
    scans = []
    for s in info.scan[:info.n_scans]:
        n = int(s.n_components)
        scans.append({'components': list(s.component)[:n], 'dc_tables': list(s.dc_table)[:n],
                      'ac_tables': list(s.ac_table)[:n], 'ss': int(s.ss), 'se': int(s.se), 'ah': int(s.ah),
                      'al': int(s.al), 'restart_interval': int(s.restart_interval), 'offset': int(s.offset),
                      'length': int(s.length), 'dc_dht': list(s.dc_dht)[:n], 'ac_dht': list(s.ac_dht)[:n]})
    d.update(scans=scans, huffman={}, progressive=True, complete=bool(info.complete))
    return d


def parse_pjpeg(data) -> dict:
    """jds_pjpeg_parse (host only, no GPU): a progressive JPEG (SOF2, 8-bit, one or three
    components) -> parse_jpeg's dict of its frame plus 'scans': the scan script in file order
    ('components', 'ss', 'se', 'ah', 'al', 'restart_interval', the byte range, and 'dc_dht' /
    'ac_dht': the file offsets of the Huffman table definitions in effect at that scan, -1 where
    it reads none) and 'complete': every coefficient is coded down to Al = 0.  ValueError naming
    the feature or the scan for anything else; a baseline file is "not progressive"."""
    a, p, n = _bytes_arg(data)
    info = _abi.PjpegInfo()
    check(lib().jds_pjpeg_parse(p, n, C.byref(info)))
    return _pjpeg_dict(info)


def decode_pjpeg(data, device: int = 0, with_status: bool = False) -> dict:
    """jds_pjpeg_decode: one progressive file -> parse_pjpeg's dict plus 'coeffs' (decode_jpeg's
    planar layout), decoded by k_pjpeg_chains: one lane per chain (all DC scans; each component's
    AC scans), scan after scan.  Defective scan data: ValueError naming the defect, or with
    with_status the dict with 'status' != 0 and unspecified coefficients."""
    a, p, n = _bytes_arg(data)
    info = _abi.PjpegInfo()
    check(lib().jds_pjpeg_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.frame.coeffs_needed), np.int16)
    with _abi.lease(device) as ctx:
        rc = lib().jds_pjpeg_decode(ctx.handle, p, n, cf.ctypes.data, cf.size, C.byref(info))
    if not (with_status and rc == _abi.JDS_EINVAL and info.status):
        check(rc)
    d = _pjpeg_dict(info)
    d['coeffs'] = cf
    d['status'] = int(info.status)
    return d


def decode_pjpeg_dev(data, coeffs_ptr: int, coeffs_cap: int, device: int = 0) -> dict:
    """jds_pjpeg_decode_dev: decode_pjpeg with the coefficients left in the caller's device buffer
    (coeffs_cap int16 entries at coeffs_ptr; entries [0, coeffs_needed) are written) -> parse_pjpeg's
    dict plus 'status' (never raises for defective scan data).  A raw pointer: the decode runs on the
    context's stream, which waits for no other, so the caller must have synchronised whatever it
    queued on that buffer (torch's fill of it, say); the call returns when the entries are written."""
    a, p, n = _bytes_arg(data)
    info = _abi.PjpegInfo()
    with _abi.lease(device) as ctx:
        rc = lib().jds_pjpeg_decode_dev(ctx.handle, p, n, C.c_void_p(int(coeffs_ptr)), int(coeffs_cap), C.byref(info))
    if not (rc == _abi.JDS_EINVAL and info.status):
        check(rc)
    d = _pjpeg_dict(info)
    d['status'] = int(info.status)
    return d


def host_decode_pjpeg(data, with_status: bool = False):
    """Test aid (jds_selftest_pjpegdec): decode_pjpeg's core on the host, chain after chain ->
    coeffs (with_status: (coeffs, status bits)).  No GPU."""
    a, p, n = _bytes_arg(data)
    info = _abi.PjpegInfo()
    check(lib().jds_pjpeg_parse(p, n, C.byref(info)))
    cf = np.empty(int(info.frame.coeffs_needed), np.int16)
    rc = lib().jds_selftest_pjpegdec(p, n, cf.ctypes.data, cf.size, C.byref(info))
    if with_status and rc == _abi.JDS_EINVAL and info.status:
        return cf, int(info.status)
    check(rc)
    return (cf, 0) if with_status else cf


def _grown(call, cap: int) -> bytes:
    """call(out array, cap, length) -> rc, repeated once with the size the C side reports."""
    n = C.c_int64(0)
    while True:
        out = np.empty(max(cap, 1), np.uint8)
        rc = call(out, cap, n)
        if rc == _abi.JDS_EINVAL and n.value > cap:
            cap = int(n.value)
            continue
        check(rc)
        return out[:n.value].tobytes()


def _encode_info(info: dict) -> _abi.JpegInfo:
    """The fields jds_encode_jpeg reads, from parse_jpeg's / decode_jpeg's terms."""
    st = _abi.JpegInfo()
    st.H, st.W, st.subsampling = int(info['H']), int(info['W']), _abi.JPEG_MODE_CODES[info['mode']]
    q = np.ascontiguousarray(info['qtables'], np.float64).reshape(3, 64)
    tq = info.get('tq', (0, 1, 1) if not info.get('single_table') else (0, 0, 0))
    for c, (gr, gc) in enumerate(info['grids']):
        st.grid_rows[c], st.grid_cols[c], st.tq[c] = int(gr), int(gc), int(tq[c])
        for i in range(64):
            st.qtable[c][i] = q[c, i]
    st.coeffs_needed = 64 * sum(int(gr) * int(gc) for gr, gc in info['grids'])
    return st


def _encode_args(coeffs, info: dict, prefix):
    st = _encode_info(info)
    cf = np.ascontiguousarray(coeffs, dtype=np.int16).reshape(-1)
    if cf.size != int(st.coeffs_needed):
        raise ValueError(f'expected {int(st.coeffs_needed)} coefficients for these block grids, got {cf.size}')
    if prefix is None:
        return st, cf, (None, None, 0)
    a = np.frombuffer(bytes(prefix), np.uint8)
    keep = a if a.size else np.zeros(1, np.uint8)   # (an empty prefix is still "a prefix": a non-null pointer)
    return st, cf, (keep, keep.ctypes.data, int(a.size))


def encode_jpeg(coeffs: np.ndarray, info: dict, optimize: bool = False, prefix=None, device: int = 0) -> bytes:
    """jds_encode_jpeg: coefficients in decode_jpeg's layout (Y, Cb, Cr planar on their T.81 grids)
    -> a baseline JPEG with ONE interleaved scan (DESIGN.md "Transcode").  info: 'H', 'W', 'mode',
    'grids', 'qtables' and 'tq' as parse_jpeg / decode_jpeg give them.  prefix: the header bytes to
    place after SOI (DQT and SOF0 among them); None: APP0, the DQTs of qtables / tq, SOF0.
    optimize: the scan's own Huffman tables instead of the Annex K ones.  ValueError for a wrong
    coefficient count, grids other than T.81's, or a block baseline JPEG cannot code."""
    st, cf, pf = _encode_args(coeffs, info, prefix)
    with _abi.lease(device) as ctx:
        return _grown(lambda out, cap, n: lib().jds_encode_jpeg(
            ctx.handle, C.byref(st), cf.ctypes.data, int(bool(optimize)), pf[1], pf[2], out.ctypes.data, cap,
            C.byref(n)), max(1 << 16, 4 * cf.size))


def host_encode_jpeg(coeffs: np.ndarray, info: dict, optimize: bool = False, prefix=None) -> bytes:
    """Test aid (jds_selftest_jpeg_encode): encode_jpeg's host model.  No GPU."""
    st, cf, pf = _encode_args(coeffs, info, prefix)
    return _grown(lambda out, cap, n: lib().jds_selftest_jpeg_encode(
        C.byref(st), cf.ctypes.data, int(bool(optimize)), pf[1], pf[2], out.ctypes.data, cap, C.byref(n)),
        max(1 << 16, 4 * cf.size))


def host_transcode_jpeg(data, optimize: bool = True) -> bytes:
    """Test aid (jds_selftest_jpeg_transcode): codec.jpeg_transcode's host model -- the host decode
    model, then the writer through the kernels' shared lookup, predecessor rule, splicer and
    table builder.  No GPU."""
    a, p, n = _bytes_arg(data)
    return _grown(lambda out, cap, m: lib().jds_selftest_jpeg_transcode(p, n, int(bool(optimize)), out.ctypes.data, cap,
                                                                        C.byref(m)), max(1 << 16, 2 * n))


def host_transform_jpeg(data, op: str = 'auto', trim: bool = False, optimize: bool = True) -> bytes:
    """Test aid (jds_selftest_jpeg_transform): codec.jpeg_transform's host model -- the host decode
    model, the host coefficient transform through the kernel's block map, the prefix editor and the
    EXIF reader (csrc/jds_xform.hpp), then the writer's host model.  No GPU."""
    a, p, n = _bytes_arg(data)
    code = _abi.xf_code(op, trim)
    return _grown(lambda out, cap, m: lib().jds_selftest_jpeg_transform(p, n, code, int(bool(optimize)), out.ctypes.data,
                                                                        cap, C.byref(m)), max(1 << 16, 2 * n))


def coef_transform_dev(coeffs: np.ndarray, info: dict, op: str, trim: bool = False, device: int = 0) -> np.ndarray:
    """Test aid (jds_selftest_coef_transform_dev): k_coef_xform alone on host coefficients in
    decode_jpeg's layout (info: 'H', 'W', 'mode', 'grids' of the source) -> the coefficients in the
    destination's layout.  op: an explicit operation."""
    st = _abi.JpegInfo()
    st.H, st.W, st.subsampling = int(info['H']), int(info['W']), _abi.JPEG_MODE_CODES[info['mode']]
    for c, (gr, gc) in enumerate(info['grids']):
        st.grid_rows[c], st.grid_cols[c] = int(gr), int(gc)
    cf = np.ascontiguousarray(coeffs, dtype=np.int16).reshape(-1)
    need = 64 * sum(int(gr) * int(gc) for gr, gc in info['grids'])
    if cf.size != need:
        raise ValueError(f'expected {need} coefficients for these block grids, got {cf.size}')
    # the destination's entries: the T.81 grids of the size after trim (a transposition keeps the count)
    hs, vs = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2), 'gray': (1, 1)}[info['mode']]
    H, W = int(info['H']), int(info['W'])
    if trim:
        if op in ('hflip', 'rot180', 'transverse', 'rot270'):
            W -= W % (8 * hs)
        if op in ('vflip', 'rot180', 'transverse', 'rot90'):
            H -= H % (8 * vs)
    n_out = 64 * (-(-H // 8) * -(-W // 8) + (0 if info['mode'] == 'gray' else 2) * (-(-(-(-H // vs)) // 8) * -(-(-(-W // hs)) // 8)))
    out = np.empty(need, np.int16)          # (never more blocks than the source has)
    with _abi.lease(device) as ctx:
        check(lib().jds_selftest_coef_transform_dev(ctx.handle, C.byref(st), _abi.xf_code(op, trim), cf.ctypes.data,
                                                    out.ctypes.data))
    return out[:n_out]


def transcode_histogram_dev(coeffs: np.ndarray, info: dict, device: int = 0) -> dict:
    """Test aid (jds_selftest_jpeg_hist_dev): the interleaved scan's symbol counts by k_mcu_hist
    -> {'dc0', 'ac0', 'dc1', 'ac1'}: counts[256]."""
    st, cf, _ = _encode_args(coeffs, info, None)
    cnt = np.zeros((2, 16 + 256), np.uint32)
    with _abi.lease(device) as ctx:
        check(lib().jds_selftest_jpeg_hist_dev(ctx.handle, C.byref(st), cf.ctypes.data, cnt.ctypes.data))
    out = {}
    for c in range(2):
        dc = np.zeros(256, np.int64)
        dc[:16] = cnt[c, :16]
        out[f'dc{c}'], out[f'ac{c}'] = dc, cnt[c, 16:].astype(np.int64)
    return out


def bitrate_from_jfif(nbytes: int, shape) -> dict:
    """bpp / compression ratio of a real file, in estimate_bitrate_no_entropy's
    terms (utils/metrics.py:62-92: 24-bit originals)."""
    h, w = shape
    bits = 8 * int(nbytes)
    return {'estimated_bits': bits, 'bpp': float(bits / (h * w)),
            'compression_ratio': float(h * w * 3 * 8 / max(bits, 1)), 'label': 'Baseline JPEG (Huffman, JFIF)'}


class PlanEntropy:
    """Device-resident entropy coding for a jds_plan: out[i] holds frame i's file.
    restart_interval (0, or restart_info()[0]): capacity, run and decode follow it.
    optimize: run() writes files with per-frame optimised tables (jds_plan_entropy_opt; its own,
    larger capacity); decode() reads only the plan's standard header and marks such files
    JDS_DEC_HEADER."""

    def __init__(self, plan: _abi.Plan, restart_interval: int = 0, optimize: bool = False):
        self.plan = plan
        self.restart_interval = int(restart_interval)
        self.optimize = bool(optimize)
        cap = C.c_int64(0)
        if self.optimize:
            check(lib().jds_plan_entropy_capacity_opt(plan.handle, self.restart_interval, C.byref(cap)))
        elif self.restart_interval:
            check(lib().jds_plan_entropy_capacity_rst(plan.handle, self.restart_interval, C.byref(cap)))
        else:
            check(lib().jds_plan_entropy_capacity(plan.handle, C.byref(cap)))
        self.capacity = int(cap.value)

    def run(self, coeffs_dev: int, out_dev: int, out_stride: int, lengths_dev: int, scan_bits_dev: int = 0,
            stream: int | None = None):
        if stream is None:
            stream = lib().jds_ctx_stream(self.plan.ctx.handle)
        if self.optimize:
            check(lib().jds_plan_entropy_opt(self.plan.handle, self.restart_interval, coeffs_dev, out_dev, out_stride,
                                             lengths_dev, scan_bits_dev or None, stream))
        elif self.restart_interval:
            check(lib().jds_plan_entropy_rst(self.plan.handle, self.restart_interval, coeffs_dev, out_dev, out_stride,
                                             lengths_dev, scan_bits_dev or None, stream))
        else:
            check(lib().jds_plan_entropy(self.plan.handle, coeffs_dev, out_dev, out_stride, lengths_dev,
                                         scan_bits_dev or None, stream))

    def decode(self, files_dev: int, stride: int, lengths_dev: int, coeffs_dev: int, status_dev: int,
               stream: int | None = None):
        """jds_plan_entropy_decode: the files run() wrote (or any with the plan's header) back to
        coefficients; status_dev: one uint32 per frame (0 = decoded).  Waits for the stream
        between propagation rounds; with a restart interval (jds_plan_entropy_decode_rst) it
        only enqueues."""
        if stream is None:
            stream = lib().jds_ctx_stream(self.plan.ctx.handle)
        if self.restart_interval:
            check(lib().jds_plan_entropy_decode_rst(self.plan.handle, self.restart_interval, files_dev, stride,
                                                    lengths_dev, coeffs_dev, status_dev, stream))
            return
        check(lib().jds_plan_entropy_decode(self.plan.handle, files_dev, stride, lengths_dev, coeffs_dev,
                                            status_dev, stream))

    def decode_rounds(self) -> int:
        """Inter-workgroup propagation rounds of the last decode()."""
        r = C.c_uint32(0)
        check(lib().jds_plan_entropy_decode_rounds(self.plan.handle, C.byref(r)))
        return int(r.value)
