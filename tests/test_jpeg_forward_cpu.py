"""CPU checks of the libjpeg encoding (no GPU; DESIGN.md "libjpeg encoding"): the NumPy definition
tests/libjpeg_fwd_ref.py against Pillow (tables and coefficients of the files it saves), the
kernel's tile core on the host (jds.codec.host_rgb_forward) against the definition, whole files
against Pillow's bytes, the division-free quantiser against //, the bad arguments, the stand-alone
sanitizer program and the exported symbols."""
import ctypes as C
import functools
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import gray_ref
import interleaved_ref as ir
import libjpeg_fwd_ref as fr
import transcode_ref as tr
from conftest import ROOT

SUBSAMPLING = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
COLOUR = list(SUBSAMPLING)
MODES = COLOUR + ['gray']
SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (37, 45), (48, 64), (50, 31), (100, 130)]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
CONTENT = ['noise', 'ramp', 'two-level']


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


@functools.lru_cache(maxsize=None)
def image(h, w, kind, seed=0):
    """HxWx3 uint8: uniform noise, ramps along both axes, or noise of 0 and 255 alone."""
    rng = np.random.default_rng([h, w, len(kind), seed])
    if kind == 'noise':
        a = rng.integers(0, 256, (h, w, 3))
    elif kind == 'two-level':
        a = rng.integers(0, 2, (h, w, 3)) * 255
    else:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(3 * x + y) % 256, (255 - 2 * y - x) % 256, (5 * x * y // (h + w) + 7 * y) % 256], -1)
    a = a.astype(np.uint8)
    a.setflags(write=False)
    return a


def of_mode(img, mode):
    return img[:, :, 1] if mode == 'gray' else img


def pillow_save(img, mode, quality, optimize=False):
    from PIL import Image
    buf = io.BytesIO()
    if mode == 'gray':
        Image.fromarray(np.ascontiguousarray(img), 'L').save(buf, 'JPEG', quality=quality, optimize=optimize)
    else:
        Image.fromarray(np.ascontiguousarray(img), 'RGB').save(buf, 'JPEG', quality=quality, optimize=optimize,
                                                              subsampling=SUBSAMPLING[mode])
    return buf.getvalue()


# --------------------------------------------- 1. the definition equals Pillow --

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', CONTENT)
def test_reference_equals_pillow(mode, kind):
    """756 cases over the parametrisation: the tables are the file's DQTs, the coefficients the
    file's on its T.81 grids."""
    for h, w in SIZES:
        for q in QUALITIES:
            img = of_mode(image(h, w, kind), mode)
            data = pillow_save(img, mode, q)
            cf, info = fr.forward(img, q, mode)
            if mode == 'gray':
                d = gray_ref.decode(data)
                assert np.array_equal(d['qtable'], fr.tables(q)[0]), (h, w, q)
                assert tuple(d['grid']) == info['grids'][0]
            else:
                d = ir.decode(data)
                assert np.array_equal(np.asarray(d['qtables'])[[0, 1]], fr.tables(q)), (h, w, q)
                assert np.array_equal(d['qtables'][2], d['qtables'][1])
                assert [tuple(g) for g in d['grids']] == info['grids']
            assert np.array_equal(np.asarray(d['planar']).reshape(-1), cf), (h, w, q)


def test_tables_call_equals_definition():
    from jds import codec
    for q in range(1, 101):
        t = codec.libjpeg_tables(q)
        assert t.shape == (2, 64) and np.array_equal(t.reshape(2, 8, 8), fr.tables(q)), q


# ------------------------------------ 2. the host core equals the definition --

EDGE_SIZES = [(h, 19) for h in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34)] + \
             [(18, w) for w in (1, 2, 3, 15, 16, 17, 127, 128, 129, 130, 257)]


@pytest.mark.parametrize('mode', MODES)
def test_host_core_equals_reference(mode):
    """Every tile edge, every odd / even case of the edge rule, a chroma plane one sample wide."""
    from jds import codec
    for h, w in EDGE_SIZES:
        for q in (1, 75, 100):
            img = of_mode(image(h, w, 'two-level' if q == 100 else 'noise', q), mode)
            cf, info = codec.host_rgb_forward(img, q, mode)
            exp, einfo = fr.forward(img, q, mode)
            assert cf.dtype == np.int16 and np.array_equal(cf, exp), (h, w, q)
            assert info['mode'] == mode and (info['H'], info['W']) == (h, w) and info['grids'] == einfo['grids']
            assert np.array_equal(info['qtables'], einfo['qtables'])
            assert list(info['tq']) == ([0, 0, 0] if mode == 'gray' else [0, 1, 1])
            assert info['coeffs_needed'] == cf.size


def test_host_core_bottom_rows_follow_the_downsampled_plane():
    """H = 18 at 4:2:0: chroma rows 9..15 of the grid repeat row 8 (pixel rows 16 and 17), not the
    image's last row alone -- with rows 16 and 17 far apart the two readings differ."""
    from jds import codec
    img = np.array(image(18, 19, 'noise'))
    img[16], img[17] = 0, 255
    cf, _ = codec.host_rgb_forward(img, 90, '4:2:0')
    assert np.array_equal(cf, fr.forward(img, 90, '4:2:0')[0])
    wrong = np.concatenate([img, np.repeat(img[17:], 14, axis=0)])      # the image padded before the downsample
    assert not np.array_equal(fr.forward(wrong, 90, '4:2:0')[0][:cf.size], cf)


# -------------------------------------------------- 3. whole files are Pillow's --

FILE_CASES = [(75, 'noise'), (95, 'two-level')]          # x 9 sizes x 3 colour modes x optimize: 108 files


@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('mode', COLOUR)
def test_files_equal_pillow(mode, optimize):
    from jds import codec, entropy
    for h, w in SIZES:
        for q, kind in FILE_CASES:
            img = image(h, w, kind)
            exp = pillow_save(img, mode, q, optimize)
            cf, info = codec.host_rgb_forward(img, q, mode)
            prefix = tr.default_prefix(h, w, mode, info['qtables'], (0, 1, 1))
            assert tr.write(cf, h, w, mode, prefix, optimize) == exp, (h, w, q)
            assert entropy.host_encode_jpeg(cf, info, optimize) == exp, (h, w, q)


@pytest.mark.parametrize('optimize', [False, True])
def test_gray_files_equal_pillow(optimize):
    from jds import codec, entropy
    for h, w in SIZES:
        for q, kind in FILE_CASES:
            img = of_mode(image(h, w, kind), 'gray')
            cf, info = codec.host_rgb_forward(img, q)
            assert info['mode'] == 'gray'
            assert entropy.host_encode_jpeg(cf, info, optimize) == pillow_save(img, 'gray', q, optimize), (h, w, q)


# ------------------------------------------------------------ 4. the division --

def test_quantiser_equals_floor_division_everywhere():
    """The core multiplies by ceil(2^20 / q): every table entry, every |c| up to the bound
    DESIGN.md derives, both signs, against //."""
    from jds import _abi
    lib = _abi.lib()
    bound = C.c_int32(0)
    one = np.zeros(2, np.int32)
    _abi.check(lib.jds_selftest_jpeg_fwd_quant(1, 1, one.ctypes.data, C.byref(bound)))
    assert bound.value >= 8200                              # |c| < 8200 for 8-bit samples
    n = bound.value + 1
    c = np.arange(n, dtype=np.int64)
    out = np.empty(2 * n, np.int32)
    for q in range(1, 256):
        _abi.check(lib.jds_selftest_jpeg_fwd_quant(q, n, out.ctypes.data, C.byref(bound)))
        exp = (c + 4 * q) // (8 * q)
        assert np.array_equal(out[:n], exp), q
        assert np.array_equal(out[n:], -exp), q


def test_coefficients_stay_below_the_bound():
    """The largest |c| before the quantiser over saturated content (flat, checkerboards, stripes
    and two-level noise) is well inside the bound the quantiser is proved for."""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:8, 0:8]
    blocks = [np.full((8, 8), v) for v in (-128, 127)]
    blocks += [np.where((x * a + y * b) % 2 == 0, 127, -128) for a, b in ((1, 0), (0, 1), (1, 1))]
    blocks += [np.where(np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16) >= 0, 127, -128)
               for u in range(8) for v in range(8)]
    blocks += list(rng.integers(0, 2, (2000, 8, 8)) * 255 - 128)
    c = fr.fdct_blocks(np.asarray(blocks, np.int64))
    assert 8000 < np.abs(c).max() < 8200


# ----------------------------------------------------------- 5. bad arguments --

def test_quality_info_arguments():
    from jds import _abi, codec
    lib = _abi.lib()
    info = _abi.JpegInfo()
    for args, name in (((0, 2, 8, 8), 'quality'), ((101, 2, 8, 8), 'quality'), ((75, 4, 8, 8), 'subsampling'),
                       ((75, -1, 8, 8), 'subsampling'), ((75, 2, 0, 8), 'H'), ((75, 2, 65536, 8), 'H'),
                       ((75, 2, 8, 0), 'W'), ((75, 0, 8, 65536), 'W')):
        assert lib.jds_jpeg_quality_info(*args, C.byref(info)) == _abi.JDS_EINVAL, args
        assert name in lib.jds_last_error().decode(), args
    assert lib.jds_jpeg_quality_info(75, 2, 65535, 17, C.byref(info)) == 0
    assert (info.grid_rows[0], info.grid_cols[0], info.grid_rows[1], info.grid_cols[1]) == (8192, 3, 4096, 2)
    assert list(info.tq) == [0, 1, 1] and info.blocks_per_mcu == 6 and info.interleaved == 1
    with pytest.raises(ValueError, match='quality'):
        codec.libjpeg_tables(0)
    with pytest.raises(ValueError, match='quality'):
        codec.host_rgb_forward(np.zeros((8, 8, 3), np.uint8), 101)
    with pytest.raises(ValueError, match='subsampling'):
        codec.host_rgb_forward(np.zeros((8, 8, 3), np.uint8), 75, '4:1:1')


def test_image_arguments():
    from jds import codec
    for bad in (np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 4), np.uint8), np.zeros((8,), np.uint8),
                np.zeros((0, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            codec.host_rgb_forward(bad)
    with pytest.raises(ValueError, match='errors'):
        codec.rgb_batch_to_jpeg([], errors='return')
    with pytest.raises(ValueError, match='out must be'):
        codec.rgb_batch_to_jpeg([], out='host')
    with pytest.raises(ValueError, match='quality values'):
        codec.rgb_batch_to_jpeg([np.zeros((8, 8, 3), np.uint8)], quality=[75, 80])


def test_forward_checks_tables_and_grids():
    """jds_jpeg_render_dev's checks: a table entry outside [1, 255] and grids that are not T.81's
    are refused before anything runs."""
    from jds import _abi, codec
    lib = _abi.lib()
    img = np.zeros((9, 9, 3), np.uint8)
    _, info = codec.host_rgb_forward(img, 75, '4:2:0')
    cf = codec._aligned_i16(info['coeffs_needed'])
    q = np.array(info['qtables'])
    q[1, 3, 3] = 256
    st = codec._jpeg_info_struct(9, 9, '4:2:0', q, info['grids'])
    with pytest.raises(ValueError, match=r'qtable\[1\]\[27\]'):
        _abi.check(lib.jds_selftest_jpeg_forward(C.byref(st), img.ctypes.data, cf.ctypes.data))
    st = codec._jpeg_info_struct(9, 9, '4:2:0', info['qtables'], [(2, 2), (2, 1), (1, 1)])
    with pytest.raises(ValueError, match='not a T.81 geometry'):
        _abi.check(lib.jds_selftest_jpeg_forward(C.byref(st), img.ctypes.data, cf.ctypes.data))
    with pytest.raises(ValueError, match='not a T.81 geometry'):        # the same checks, before the context is looked at
        _abi.check(lib.jds_jpeg_forward_dev(None, C.byref(st), None, None, None))


# ---------------------------------------------------------- 6. build and ABI --

def test_new_symbols_and_abi_version():
    from jds import _abi
    lib = _abi.lib()
    assert lib.jds_abi_version() == 3
    for name in ('jds_jpeg_quality_info', 'jds_jpeg_forward_dev', 'jds_rgb_to_jpeg', 'jds_rgb_batch_to_jpeg',
                 'jds_selftest_jpeg_forward', 'jds_selftest_jpeg_fwd_quant'):
        assert hasattr(lib, name), name
    from jds import build
    assert 'jds_jpeg_fwd.hip' in build.SOURCES and 'jds_jpeg_fwd.hpp' in build.headers()


def test_tile_core_clean_under_host_sanitizers(tmp_path):
    """tools/jpeg_fwd_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: the host tile loop against a plain whole-plane implementation
    over every size up to 40 x 40 in the four modes, noise and two-level noise, from exactly-sized
    heap arrays."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'jpeg_fwd_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'jpeg_fwd_san.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stderr == '', r.stderr[-4000:]
    images, checks, failed = (int(r.stdout.split()[i]) for i in (0, 2, 4))
    assert images >= 4 * 40 * 40 * 2 and checks > images and failed == 0
