"""CPU checks of the lossless transforms (DESIGN.md "Lossless transforms"; no GPU): the
definition (tests/transform_ref.py) against itself and against Pillow's pixels, the host model
(jds_selftest_jpeg_transform: host decode model, the coefficient transform through the kernel's
block map, the prefix editor and EXIF reader of csrc/jds_xform.hpp, the writer's host model)
against the definition byte for byte, trim and refusals, the sanitizer program and the ABI."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageOps

import interleaved_ref as il
import transcode_cases as tc
import transcode_ref as tr
import transform_cases as xc
import transform_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_IDS = [f'{h}x{w}-{m}' for h, w, m, _ in xc.SIZES]
FOREIGN_IDS = [f'{c[0]}x{c[1]}-{c[2]}-ri{c[6]}-{"3scan" if c[7] else "il"}-s{c[3]}' for c in tc.FOREIGN_CASES]


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def host(data, op, optimize=True, trim=False):
    from jds import entropy
    return entropy.host_transform_jpeg(data, op, trim=trim, optimize=optimize)


# -------------------------------------------- 1. the reference against itself --

@pytest.mark.parametrize('h,w,mode,ops', xc.SIZES, ids=SIZE_IDS)
def test_reference_round_trips(h, w, mode, ops):
    for optimize in (False, True):
        src = tc.pillow(h, w, mode, 50, False, True)
        same = tr.transcode(src, optimize)
        t = lambda d, op: xr.transform(d, op, False, optimize)
        if 'hflip' in ops:
            assert t(t(src, 'hflip'), 'hflip') == same
            assert t(t(src, 'vflip'), 'vflip') == same
            assert t(t(src, 'rot180'), 'rot180') == same
        if 'rot90' in ops:
            assert t(t(src, 'rot90'), 'rot270') == same
            assert t(src, 'rot90') == t(t(src, 'transpose'), 'hflip')
            assert t(src, 'rot270') == t(t(src, 'hflip'), 'transpose')
            assert t(src, 'transverse') == t(t(src, 'transpose'), 'rot180')
        if 'transpose' in ops:
            once = t(src, 'transpose')
            assert once != same and t(once, 'transpose') == same
            d = il.decode(once)
            assert (d['H'], d['W'], d['mode']) == (w, h, mode)
        assert t(src, 'none') == same


# ----------------------------------------------------- 2. orientation sense --

def _pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


@pytest.mark.parametrize('op', xc.OPS)
def test_orientation_sense_of_each_operation(op):
    """Pinned by Pillow's pixels and NumPy's rot90 / flips, not by the reference's own arithmetic."""
    src = xc.quadrant_file()
    px = _pixels(src)
    for out in (xr.transform(src, op, False, True), host(src, op)):
        best, d, others = xc.closest_orientation(px, _pixels(out))
        print(f'{op}: closest {best}, difference {d:.4f}, next {others:.4f}')
        assert best == op and d < others / 10
    assert tc.ICC in out and tc.COMMENT in out


@pytest.mark.parametrize('big', [True, False], ids=['MM', 'II'])
@pytest.mark.parametrize('orientation', range(1, 9))
def test_auto_orient_against_pillow(orientation, big):
    src = xc.quadrant_file(xc.exif_block(orientation, big))
    im = Image.open(io.BytesIO(src))
    assert im.getexif()[0x0112] == orientation
    want = np.asarray(ImageOps.exif_transpose(im).convert('RGB'))
    px = _pixels(src)
    intended = [k for k, f in xc.ORIENT.items() if f(px).shape == want.shape and np.array_equal(f(px), want)]
    assert intended == [xr.ORIENTATION[orientation]]
    ref = xr.transform(src, 'auto', False, True)
    got = host(src, 'auto')
    assert got == ref
    out = Image.open(io.BytesIO(got))
    assert out.getexif()[0x0112] == 1
    best, d, others = xc.closest_orientation(px, np.asarray(out.convert('RGB')))
    print(f'orientation {orientation}: closest {best}, difference {d:.4f}, next {others:.4f}')
    assert best == intended[0] and d < others / 10
    assert tc.ICC in got and tc.COMMENT in got
    assert out.info.get('icc_profile') == tc.ICC
    # an explicit operation never touches the tag
    assert Image.open(io.BytesIO(host(src, 'hflip'))).getexif()[0x0112] == orientation


# --------------------------------------------------------- 3. the host model --

@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('h,w,mode,ops', xc.SIZES, ids=SIZE_IDS)
def test_host_model_equals_reference(h, w, mode, ops, optimize):
    src = tc.pillow(h, w, mode, 50, False, True)
    for op in ops:
        assert host(src, op, optimize) == xr.transform(src, op, False, optimize), op
    from jds import entropy
    assert host(src, 'none', optimize) == entropy.host_transcode_jpeg(src, optimize) == tr.transcode(src, optimize)


@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('case', tc.FOREIGN_CASES, ids=FOREIGN_IDS)
def test_host_model_on_foreign_files(case, optimize):
    """Foreign table assignments, three quantisation tables (an untransposed DQT shows), restart
    files, three-scan files: the operations the size allows, and all the mode allows with trim."""
    src = tc.foreign(*case)
    h, w, mode = case[:3]
    ran = 0
    for trim in (False, True):
        for op in xc.allowed(h, w, mode, trim):
            got = host(src, op, optimize, trim)
            assert got == xr.transform(src, op, trim, optimize), (op, trim)
            ran += 1
            if op in xr.TRANSPOSING:
                d0, d1 = il.decode(src), il.decode(got)
                assert all(np.array_equal(d1['qt'][i], d0['qt'][i].T) for i in d0['qt'])
                assert d1['tq'] == d0['tq']
    assert ran >= (3 if mode == '4:2:2' else 7)


def test_three_distinct_tables_are_each_transposed():
    case = tc.FOREIGN_CASES[1]
    assert case[5] == (0, 1, 2)
    src = tc.foreign(*case)
    d0, d1 = il.decode(src), il.decode(host(src, 'transpose'))
    assert len(d0['qt']) == 3 and not np.array_equal(d0['qt'][1], d0['qt'][2])
    for i in range(3):
        assert not np.array_equal(d0['qt'][i], d0['qt'][i].T)        # the case cannot pass untransposed
        assert np.array_equal(d1['qt'][i], d0['qt'][i].T)


# ------------------------------------------------------ 4. trim and refusals --

def test_trim_and_refusals():
    from jds import codec
    f = tc.pillow(37, 53, '4:2:0', 50, False, True)
    with pytest.raises(ValueError, match=r'width 53 is not a multiple of 16'):
        host(f, 'hflip')
    with pytest.raises(ValueError, match=r'width 53 is not a multiple of 16'):
        codec.jpeg_transform_info(f, 'hflip')
    with pytest.raises(xr.NotSupported):
        xr.transform(f, 'hflip', False, True)
    got = host(f, 'hflip', trim=True)
    assert got == xr.transform(f, 'hflip', True, True)
    d = il.decode(got)
    assert (d['H'], d['W']) == (37, 48)
    assert codec.jpeg_transform_info(f, 'hflip', trim=True) == {'op': 'hflip', 'H': 37, 'W': 48}
    assert codec.jpeg_transform_info(f, 'rot90', trim=True) == {'op': 'rot90', 'H': 53, 'W': 32}
    assert codec.jpeg_transform_info(f, 'transpose') == {'op': 'transpose', 'H': 53, 'W': 37}
    with pytest.raises(ValueError, match=r'height 37 is not a multiple of 16'):
        host(f, 'rot90')
    g = tc.pillow(32, 48, '4:2:2', 50, False, True)
    for fn in (lambda: host(g, 'rot90'), lambda: codec.jpeg_transform_info(g, 'rot90'),
               lambda: host(g, 'transpose', trim=True)):
        with pytest.raises(ValueError, match=r'4:2:2 takes only hflip, vflip and rot180'):
            fn()
    with pytest.raises(xr.NotSupported):
        xr.transform(g, 'rot90', False, True)
    e = tc.pillow(7, 200, '4:2:0', 50, False, False)
    for fn in (lambda: host(e, 'vflip', trim=True), lambda: codec.jpeg_transform_info(e, 'vflip', trim=True)):
        with pytest.raises(ValueError, match='trim leaves nothing'):
            fn()
    with pytest.raises(xr.Empty):
        xr.transform(e, 'vflip', True, True)
    # the error codes behind the messages
    from jds import _abi
    a = np.frombuffer(f, np.uint8)
    op, H, W = C.c_int32(), C.c_int64(), C.c_int64()
    args = (C.byref(op), C.byref(H), C.byref(W))
    assert _abi.lib().jds_jpeg_transform_info(a.ctypes.data, a.size, 1, *args) == _abi.JDS_ENOTSUP
    a = np.frombuffer(g, np.uint8)
    assert _abi.lib().jds_jpeg_transform_info(a.ctypes.data, a.size, 5, *args) == _abi.JDS_ENOTSUP
    a = np.frombuffer(e, np.uint8)
    assert _abi.lib().jds_jpeg_transform_info(a.ctypes.data, a.size, 2 | 0x100, *args) == _abi.JDS_EINVAL


@pytest.mark.parametrize('exif', [None, xc.exif_block(6, True, count_lie=5), xc.exif_block(9), xc.exif_block(0),
                                  xc.exif_block(6, False, tag_type=4), b'Exif\x00\x00MM\x00\x2a\x00\x00\x00\x50',
                                  b'Exif\x00\x00XX\x00\x2a\x00\x00\x00\x08\x00\x00'],
                         ids=['none', 'truncated-ifd', 'value-9', 'value-0', 'type-long', 'ifd-outside', 'byte-order'])
def test_auto_without_usable_orientation_is_the_plain_transcode(exif):
    from jds import codec
    src = xc.quadrant_file(exif)
    assert (b'Exif' in src) == (exif is not None)
    want = tr.transcode(src, True)
    assert xr.transform(src, 'auto', False, True) == want
    assert host(src, 'auto') == want
    assert codec.jpeg_transform_info(src, 'auto') == {'op': 'none', 'H': 48, 'W': 80}


# ------------------------------------------------------------- 5. sanitizers --

def test_prefix_editor_and_exif_reader_under_sanitizers(tmp_path):
    """tools/jpeg_xform_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined."""
    cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++')
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'jpeg_xform_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'jpeg_xform_san.cpp'), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'ok' in r.stdout


# -------------------------------------------------------------------- 6. ABI --

def test_abi_symbols_and_argument_checks():
    from jds import _abi, codec, entropy
    L = _abi.lib()
    for name in ('jds_jpeg_transform_info', 'jds_jpeg_transform', 'jds_jpeg_batch_transform',
                 'jds_selftest_jpeg_transform', 'jds_selftest_coef_transform_dev'):
        assert hasattr(L, name), name
    f = tc.pillow(16, 16, '4:2:0', 50, False, True)
    a = np.frombuffer(f, np.uint8)
    n, op, H, W = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
    buf = np.empty(1 << 16, np.uint8)
    assert L.jds_jpeg_transform_info(None, a.size, 1, C.byref(op), C.byref(H), C.byref(W)) == _abi.JDS_EINVAL
    assert L.jds_jpeg_transform_info(a.ctypes.data, a.size, 1, None, C.byref(H), C.byref(W)) == _abi.JDS_EINVAL
    assert L.jds_selftest_jpeg_transform(None, a.size, 1, 1, buf.ctypes.data, buf.size, C.byref(n)) == _abi.JDS_EINVAL
    assert L.jds_selftest_jpeg_transform(a.ctypes.data, a.size, 1, 1, buf.ctypes.data, buf.size, None) == _abi.JDS_EINVAL
    assert L.jds_jpeg_transform(None, a.ctypes.data, a.size, 1, 1, buf.ctypes.data, buf.size, C.byref(n), None) \
        == _abi.JDS_EINVAL
    assert L.jds_jpeg_batch_transform(None, None, None, 0, None, 1, None, 0, 0, None, C.byref(n)) == _abi.JDS_EINVAL
    assert L.jds_selftest_coef_transform_dev(None, None, 1, None, None) == _abi.JDS_EINVAL
    for bad in (9, 0x200 | 1, -1, 0x109):
        assert L.jds_selftest_jpeg_transform(a.ctypes.data, a.size, bad, 1, buf.ctypes.data, buf.size, C.byref(n)) \
            == _abi.JDS_EINVAL
        assert b'unknown transform operation' in L.jds_last_error()
        assert L.jds_jpeg_transform_info(a.ctypes.data, a.size, bad, C.byref(op), C.byref(H), C.byref(W)) \
            == _abi.JDS_EINVAL
    with pytest.raises(ValueError, match='unknown transform operation'):
        entropy.host_transform_jpeg(f, 'rot45')
    with pytest.raises(ValueError, match='unknown transform operation'):
        codec.jpeg_transform_info(f, 'flip')
    # a short buffer names the need
    rc = L.jds_selftest_jpeg_transform(a.ctypes.data, a.size, 1, 1, buf.ctypes.data, 10, C.byref(n))
    assert rc == _abi.JDS_EINVAL and n.value == len(host(f, 'hflip'))
