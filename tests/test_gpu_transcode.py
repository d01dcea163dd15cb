"""GPU checks of the lossless transcode (csrc/jds_entropy_mcu.hip: the interleaved-scan writer
behind jds_jpeg_transcode, jds_jpeg_batch_transcode and jds_encode_jpeg).  The yardsticks are the
definition (tests/transcode_ref.py), Pillow (libjpeg) wherever Pillow made the input -- its
plain and optimize=True files of one image are each other's transcodes -- and the host model."""
import io

import numpy as np
import pytest
from PIL import Image

import huffopt_ref as hr
import interleaved_ref as ir
import transcode_cases as tc
import transcode_ref as tr
from test_jpeg_batch_cpu import flipped

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def dev(data, optimize):
    from jds import codec
    return codec.jpeg_transcode(data, optimize=optimize)


# ------------------------------------------------------ 1. against the reference --

SMALL = [(h, w, m) for (h, w) in [(1, 1), (17, 33), (37, 53)] for m in tc.MODES]
# 200 x 264 at 4:2:0: 13 x 17 MCUs of 6 = 1326 scan blocks, 21 segments, no MCU ends on a segment
# boundary but every 32nd, padding on both edges; 264 x 200 likewise at 4 and 3 blocks per MCU
MEDIUM = [(200, 264, '4:2:0'), (264, 200, '4:2:2'), (264, 200, '4:4:4')]


@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('h,w,mode', SMALL + MEDIUM)
def test_gpu_transcode_against_reference_and_pillow(h, w, mode, optimize):
    plain, opt = tc.pillow(h, w, mode, 50, False, True), tc.pillow(h, w, mode, 50, True, True)
    src, want = (plain, opt) if optimize else (opt, plain)
    got = dev(src, optimize)
    assert got == want                                   # Pillow's own file of the other kind
    if (h, w, mode) == MEDIUM[0]:
        d = ir.decode(src)
        assert 6 * d['mcu'][0] * d['mcu'][1] == 1326 and d['padded'][0].shape[:2] != d['grids'][0]
    assert got == tr.transcode(src, optimize)
    assert dev(want, optimize) == want                   # the identity on a file of the target kind


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_foreign_files_against_reference(optimize):
    for case in tc.FOREIGN_CASES:
        src = tc.foreign(*case)
        got = dev(src, optimize)
        assert got == tr.transcode(src, optimize), case
        assert np.array_equal(ir.decode(got)['planar'], ir.decode(src)['planar'])


# ----------------------------------------------------------- 2. long-scan route --

@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_long_scan_route(optimize):
    """1080 x 1920 at 4:2:0: 68 x 120 MCUs = 48,960 scan blocks, 765 segments: past the length a
    scan sums its own segment totals at, so the per-file prefix launch runs."""
    h, w, mode = 1080, 1920, '4:2:0'
    plain, opt = tc.pillow(h, w, mode, 50, False, True), tc.pillow(h, w, mode, 50, True, True)
    src, want = (plain, opt) if optimize else (opt, plain)
    from jds import entropy
    m = entropy.parse_jpeg(src)['mcu']
    assert m['rows'] * m['cols'] * m['blocks'] == 48960 and -(-48960 // 64) == 765 > 512
    assert dev(src, optimize) == want


# ------------------------------------------------------------- 3. mixed batch --

def mixed_batch():
    """(files, indices of the good ones, index of the rejected one, index of the corrupt one)."""
    from jds import entropy
    h, w, mode = 48, 64, '4:2:0'
    own = entropy.encode_jfif(tc.random_coeffs(h, w, mode, 3), h, w, mode, tc.Q50, optimize=True)[0]
    b = io.BytesIO()
    Image.fromarray(tc.image(24, 24)).save(b, 'JPEG', progressive=True)
    files = [tc.pillow(1, 1, '4:4:4', 50, False, True),
             tc.pillow(200, 264, '4:2:0', 50, False, True),
             tc.pillow(37, 53, '4:2:2', 92, True, False),
             b.getvalue(),                                           # 3: the parser rejects it
             tc.pillow(100, 75, '4:2:0', 50, False, True, restart_rows=1),
             tc.foreign(*tc.FOREIGN_CASES[1]),
             flipped(tc.pillow(37, 53, '4:2:0', 50, False, False)),  # 6: a corrupted scan
             own,                                                    # 7: three scans, this library's
             tc.pillow(264, 200, '4:4:4', 50, False, False),
             tc.foreign(*tc.FOREIGN_CASES[4]),                       # restart intervals, padding
             tc.pillow(17, 33, '4:2:0', 50, False, True),
             tc.foreign(*tc.FOREIGN_CASES[7])]                       # three scans with restart intervals
    return files, [i for i in range(len(files)) if i not in (3, 6)], 3, 6


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_mixed_batch(optimize):
    import torch
    from jds import codec
    files, good, rejected, corrupt = mixed_batch()
    outs, items = codec.jpeg_batch_transcode(files, optimize=optimize, errors='items')
    assert [i for i, o in enumerate(outs) if o is not None] == good
    assert items[rejected]['rc'] != 0 and items[rejected]['out_len'] == 0 and items[rejected]['out_off'] == -1
    assert items[corrupt]['rc'] == 0 and items[corrupt]['status'] != 0 and items[corrupt]['out_len'] == 0
    off = 0
    for i in good:                                       # packed in batch order, each at a multiple of 256
        assert items[i]['out_off'] == off and items[i]['out_len'] == len(outs[i])
        off = -(-(off + len(outs[i])) // 256) * 256
    for i in good:
        assert outs[i] == dev(files[i], optimize), i     # the single call
        assert outs[i] == tr.transcode(files[i], optimize), i
    with pytest.raises(ValueError, match=rf'file {rejected}: .*progressive'):
        codec.jpeg_batch_transcode(files, optimize=optimize)
    # on the device, into a pre-filled buffer: the same bytes, the gaps untouched
    buf = torch.full((off + 512,), 0xA5, dtype=torch.uint8, device='cuda:0')
    views, items_d = codec.jpeg_batch_transcode(files, optimize=optimize, out=buf, errors='items')
    assert items_d == items
    host = buf.cpu().numpy()
    end = 0
    for i in good:
        o, n = items[i]['out_off'], items[i]['out_len']
        assert np.all(host[end:o] == 0xA5)
        assert host[o:o + n].tobytes() == outs[i] == views[i].cpu().numpy().tobytes()
        end = o + n
    assert np.all(host[end:] == 0xA5)
    # the neighbours do not depend on the bad files
    alone, _ = codec.jpeg_batch_transcode([files[i] for i in good], optimize=optimize, errors='items')
    assert alone == [outs[i] for i in good]
    # a buffer that is too small names the need and writes nothing
    small = torch.full((off - 256,), 0xA5, dtype=torch.uint8, device='cuda:0')
    with pytest.raises(ValueError, match=str(off)):
        codec.jpeg_batch_transcode(files, optimize=optimize, out=small, errors='items')
    assert bool((small == 0xA5).all())


def test_gpu_empty_batch():
    from jds import codec
    assert codec.jpeg_batch_transcode([]) == []
    assert codec.jpeg_batch_transcode([], out='device', errors='items') == ([], [])


# --------------------------------------------------------------- 4. round trip --

@pytest.mark.parametrize('h,w,mode', [(37, 53, '4:2:0'), (200, 264, '4:2:0'), (264, 200, '4:2:2'), (17, 33, '4:4:4')])
def test_gpu_round_trip(h, w, mode):
    from jds import codec, entropy
    for src in (tc.pillow(h, w, mode, 92, False, True), tc.foreign(h, w, mode, 9, ((1, 1), (0, 0), (0, 1)), (0, 1, 2))):
        out = dev(src, True)
        assert np.array_equal(codec.jpeg_to_rgb(out), codec.jpeg_to_rgb(src))
        a, b = entropy.decode_jpeg(out), entropy.decode_jpeg(src)
        assert np.array_equal(a['coeffs'], b['coeffs']) and a['grids'] == b['grids']
        assert a['interleaved'] and a['scans'][0]['restart_interval'] == 0


# ------------------------------------------------------ 5. host model agreement --

def test_gpu_not_codable_agrees_with_host_model():
    from jds import codec, entropy
    src = tc.not_codable()
    assert np.array_equal(entropy.decode_jpeg(src)['coeffs'], ir.decode(src)['planar'])
    for optimize in (False, True):
        with pytest.raises(ValueError, match='not baseline-codable'):
            entropy.host_transcode_jpeg(src, optimize)
        with pytest.raises(ValueError, match='not baseline-codable'):
            dev(src, optimize)
    good = tc.pillow(17, 33, '4:2:0', 50, False, True)
    outs, items = codec.jpeg_batch_transcode([good, src, good], errors='items')
    assert outs[1] is None and items[1]['rc'] != 0 and items[1]['out_len'] == 0
    assert outs[0] == outs[2] == dev(good, True) and items[2]['out_off'] == -(-len(outs[0]) // 256) * 256
    with pytest.raises(ValueError, match='file 1: not baseline-codable'):
        codec.jpeg_batch_transcode([good, src, good])


def test_gpu_single_calls_report_and_take_the_exact_length():
    """The single calls run the batch writer packed at 1, not at 256: a buffer of exactly the
    file's length suffices, and one byte less is JDS_EINVAL with *out_len the exact length
    (jds_jpeg_transcode; jds_rgb_to_jpeg on a 16 x 16 image)."""
    import ctypes as C
    from jds import _abi, entropy
    lib = _abi.lib()
    src = tc.pillow(17, 33, '4:2:0', 50, False, True)
    a, p, n = entropy._bytes_arg(src)
    info = _abi.JpegInfo()
    img = np.random.default_rng(16).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=75, subsampling=2)      # (what jds_rgb_to_jpeg writes, byte for byte)
    pil = buf.getvalue()
    with _abi.lease(0) as ctx:
        calls = ((entropy.host_transcode_jpeg(src, True),
                  lambda o, cap, m: lib.jds_jpeg_transcode(ctx.handle, p, n, 1, o.ctypes.data, cap, C.byref(m), C.byref(info))),
                 (pil,
                  lambda o, cap, m: lib.jds_rgb_to_jpeg(ctx.handle, C.c_void_p(img.ctypes.data), 0, 16, 16, 75,
                                                        _abi.JPEG_MODE_CODES['4:2:0'], 0, o.ctypes.data, cap, C.byref(m))))
        for want, call in calls:
            assert len(want) % 256                           # (the batch's packing would ask for more)
            out, m = np.full(len(want), 0xA5, np.uint8), C.c_int64(-1)
            assert call(out, len(want) - 1, m) == _abi.JDS_EINVAL and m.value == len(want)
            assert 'output buffer too small: %d bytes needed' % len(want) in lib.jds_last_error().decode()
            assert bool((out == 0xA5).all())
            m = C.c_int64(-1)
            assert call(out, len(want), m) == 0 and m.value == len(want) and out.tobytes() == want


def test_gpu_stuffing_agrees_with_host_model():
    from jds import entropy
    src = tc.pillow(64, 48, '4:2:0', 100, False, False, noise=True)
    assert ir.decode(src)['segment'].count(b'\xff\x00') > 20
    for optimize in (False, True):
        got = dev(src, optimize)
        assert got == entropy.host_transcode_jpeg(src, optimize)
        assert got == tc.pillow(64, 48, '4:2:0', 100, optimize, False, noise=True)


def test_gpu_encode_from_raw_coefficients():
    from jds import entropy
    for h, w, mode in [(1, 1, '4:2:0'), (17, 33, '4:2:2'), (40, 24, '4:4:4'), (37, 53, '4:2:0')]:
        cf, info = tc.random_coeffs(h, w, mode, 5 + h), tc.info_of(h, w, mode)
        for optimize in (False, True):
            got = entropy.encode_jpeg(cf, info, optimize=optimize)
            assert got == entropy.host_encode_jpeg(cf, info, optimize=optimize)
            assert np.array_equal(ir.decode(got)['planar'], cf)
    cf, info, _ = tc.k3_coeffs()                         # K.3 shortens this scan's AC luma codes
    got = entropy.encode_jpeg(cf, info, optimize=True)
    assert got == entropy.host_encode_jpeg(cf, info, optimize=True)
    assert max(i + 1 for i, b in enumerate(hr.file_tables(got)['ac0'][0]) if b) == 16
    with pytest.raises(ValueError, match='coefficients'):
        entropy.encode_jpeg(cf[:-64], info)
    with pytest.raises(ValueError, match='T.81'):
        entropy.encode_jpeg(np.zeros(64 * 19, np.int16), dict(tc.info_of(17, 33, '4:2:0'), grids=[(3, 5), (1, 2), (1, 2)]))


# ---------------------------------------------------- 6. interleaved histogram --

def test_gpu_interleaved_histogram():
    from jds import entropy
    src = tc.pillow(200, 264, '4:2:0', 50, False, True)
    d = ir.decode(src)
    want = tr.scan_histograms(tr.dummy_padded(d['planar'], 200, 264, '4:2:0'), 200, 264, '4:2:0')
    got = entropy.transcode_histogram_dev(d['planar'], tc.info_of(200, 264, '4:2:0'))
    for k in hr.CLASSES:
        assert np.array_equal(got[k], want[k]), k
    n_pad = 6 * 13 * 17 - sum(r * c for r, c in d['grids'])
    assert n_pad > 0 and want['dc0'].sum() == 4 * 13 * 17   # the padding blocks' symbols are counted
