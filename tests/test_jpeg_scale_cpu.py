"""CPU checks of the scaled libjpeg rendering (no GPU; DESIGN.md "Scaled libjpeg rendering"): the
NumPy definition tests/libjpeg_scaled_ref.py against Pillow's Image.draft byte for byte, the
kernel's tile core on the host (jds_selftest_jpeg_render_scaled) against the definition, the host
model of a batch with mixed denominators, the arguments, and the stand-alone sanitizer program."""
import functools
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import libjpeg_scaled_ref as ls
from conftest import ROOT
from test_jpeg_render_cpu import _decoded, hostile, pillow_file, tile_sizes

DENOMS = (2, 4, 8)
MODES = ['4:4:4', '4:2:2', '4:2:0', 'L']
BASE_SIZES = [(3, 5), (8, 8), (9, 17), (15, 23), (17, 33), (37, 53), (48, 130)]
# 4:2:2: the cropped chroma plane is ceil(W * m / 16) wide, m = 8 / d.  1, 2 and 3 samples at
# d = 2: W = 4, 8, 12 (and 3, 7, 9, not multiples of d); d = 4: W = 8, 16, 24 (and 7, 14, 18);
# d = 8: W = 16, 32, 48 (and 9, 31, 33).  Two samples or fewer replicate, three take the taps.
NARROW_SIZES = [(9, w) for w in (3, 4, 7, 8, 9, 12, 14, 16, 18, 24, 31, 32, 33, 48)]
ODD_SIZES = [(10, 13), (11, 25), (13, 47), (21, 19)]         # no side a multiple of 8, 4 or (but one) 2
SMALL_SIZES = [(1, 1), (3, 5), (5, 3), (7, 130)]             # a side below the denominator: no draft


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def contents(mode):
    """A picture and a saturating noise file; 4:2:0 at a second quality."""
    return [(90, 'picture'), (100, 'noise')] + ([(30, 'picture')] if mode == '4:2:0' else [])


def sizes():
    return list(dict.fromkeys(BASE_SIZES + tile_sizes() + NARROW_SIZES + ODD_SIZES))


def draft_pixels(data, denom):
    """Pillow's reduced decode: draft(mode, (W // d, H // d)) selects exactly d when both sides
    are at least d."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    assert w >= denom and h >= denom
    im.draft(im.mode, (w // denom, h // denom))
    assert im.decoderconfig[0] == denom
    return np.asarray(im.convert('RGB'))


@functools.lru_cache(maxsize=None)
def model(data, denom):
    """libjpeg_scaled_ref.render_scaled of a file, computed once and shared (read-only)."""
    img = ls.render_scaled(*_decoded(data), denom)
    img.setflags(write=False)
    return img


def host_scaled(data, denom):
    from jds import codec
    return codec.host_jpeg_render(*_decoded(data), render='libjpeg', scale_denom=denom)


# ------------------------------------------- 1. the definition equals Pillow --

@pytest.mark.parametrize('mode', MODES)
def test_model_equals_pillow_draft(mode):
    compared = 0
    for h, w in sizes():
        for q, kind in contents(mode):
            data = pillow_file(h, w, mode, q, kind)
            for d in DENOMS:
                if h < d or w < d:
                    continue                                 # (test 2 takes these)
                exp = draft_pixels(data, d)
                got = model(data, d)
                assert got.shape == exp.shape == (-(-h // d), -(-w // d), 3), (h, w, d)
                assert np.array_equal(got, exp), (mode, h, w, q, kind, d)
                compared += 1
    assert compared >= 3 * len(contents(mode)) * (len(sizes()) - 3)


# --------------------------------------- 2. the host core equals the definition --

@pytest.mark.parametrize('mode', MODES)
def test_host_core_equals_model(mode):
    for h, w in sizes() + SMALL_SIZES:
        for q, kind in contents(mode):
            data = pillow_file(h, w, mode, q, kind)
            for d in DENOMS:
                got = host_scaled(data, d)
                assert got.dtype == np.uint8 and got.shape == (-(-h // d), -(-w // d), 3)
                assert np.array_equal(got, model(data, d)), (mode, h, w, q, kind, d)


def test_below_denominator_sizes():
    """A 3 x 5 file at 1/8 is 1 x 1; a 7 x 130 one is 1 x 17."""
    from jds import codec
    assert host_scaled(pillow_file(3, 5, '4:2:0'), 8).shape == (1, 1, 3)
    assert host_scaled(pillow_file(7, 130, '4:2:2'), 8).shape == (1, 17, 3)
    assert codec.jpeg_scaled_size(3, 5, 8) == (1, 1) and codec.jpeg_scaled_size(7, 130, 4) == (2, 33)


@pytest.mark.parametrize('mode', ['4:4:4', '4:2:2', '4:2:0', 'gray'])
def test_hostile_coefficients_core_equals_model(mode):
    from jds import codec
    th, tw = codec.jpeg_inverse_info()
    for seed, (h, w) in enumerate([(1, 1), (9, 9), (31, 45), (th + 1, tw + 1)]):
        args = hostile(h, w, mode, seed)
        for d in DENOMS:
            exp = ls.render_scaled(*args, d)
            assert np.array_equal(codec.host_jpeg_render(*args, render='libjpeg', scale_denom=d), exp), (h, w, d)


# ------------------------------------------------------ 3. host batch model --

def mixed_batch():
    """(files, denominators): the modes and the denominators mixed, 1 among them, a file the
    parser rejects (index 3) and one whose scan data are defective (index 6)."""
    from test_jpeg_batch_cpu import flipped
    from test_jpeg_interleaved_cpu import fixture
    files = [pillow_file(31, 45, '4:2:0'), pillow_file(9, 9, '4:4:4'), pillow_file(7, 9, 'L'),
             b'\xff\xd8\xff\xe0\x00\x02not a jpeg', pillow_file(33, 129, '4:2:2'), fixture('p40x72_420_rst2')[0],
             flipped(fixture('p24x40_420')[0]), pillow_file(37, 53, 'L'), pillow_file(3, 4, '4:2:0'),
             pillow_file(65, 257, '4:2:0', 30), pillow_file(33, 129, '4:2:2'), pillow_file(17, 33, '4:4:4'),
             pillow_file(31, 45, '4:2:0')]
    return files, [2, 4, 1, 2, 2, 8, 4, 8, 8, 4, 1, 2, 1]


def test_host_batch_model_mixed_denominators():
    from jds import codec
    from test_jpeg_render_cpu import host_render
    files, dens = mixed_batch()
    rgb, cf, items = codec.host_jpeg_batch(files, render='libjpeg', scale_denom=dens)
    lay, rgb_bytes, _ = codec.jpeg_batch_layout(files, scale_denom=dens)
    assert rgb_bytes == rgb.size and [it['rgb_off'] for it in lay] == [it['rgb_off'] for it in items]
    assert [it['rc'] == 0 for it in items] == [i != 3 for i in range(len(files))]
    assert items[3]['rgb_off'] == -1 and items[6]['status'] != 0
    covered = np.zeros(rgb.size, bool)
    end = 0
    for i, (f, d, it) in enumerate(zip(files, dens, items)):
        assert it['scale_denom'] == d
        if it['rc'] != 0:
            continue
        assert (it['out_H'], it['out_W']) == codec.jpeg_scaled_size(it['H'], it['W'], d)
        o, n = it['rgb_off'], it['out_H'] * it['out_W'] * 3
        assert o % 256 == 0 and o == -(-end // 256) * 256      # batch order, the next multiple of 256
        end = o + n
        covered[o:o + n] = True
        img = rgb[o:o + n].reshape(it['out_H'], it['out_W'], 3)
        if it['status']:
            assert not img.any(), i                         # a defective scan: zeros over its scaled image
            continue
        assert np.array_equal(img, host_scaled(f, d) if d != 1 else host_render(f)), i
        assert np.array_equal(img, model(f, d)), i
    assert covered.any() and not covered.all() and np.all(rgb[~covered] == 0xA5)   # the guard bytes keep the fill


# ------------------------------------------------------------ 4. arguments --

def test_bad_denominators_and_scaled_reference_are_value_errors():
    import ctypes as C
    from jds import _abi, codec
    data = pillow_file(9, 9, '4:2:0')
    d = _decoded(data)
    info = {'H': 9, 'W': 9, 'mode': d[3], 'qtables': d[4], 'grids': d[5]}
    for bad in (0, 3, 16, -2, 2.0, '2', None, True):
        with pytest.raises(ValueError, match='scale_denom'):
            codec.host_jpeg_render(*d, render='libjpeg', scale_denom=bad)
        with pytest.raises(ValueError, match='scale_denom'):
            codec.host_jpeg_batch([data], render='libjpeg', scale_denom=bad)
        with pytest.raises(ValueError, match='scale_denom'):
            codec.jpeg_to_rgb(data, render='libjpeg', scale_denom=bad)
        with pytest.raises(ValueError, match='scale_denom'):
            codec.jpeg_batch_to_rgb([data], render='libjpeg', scale_denom=[bad])
        with pytest.raises(ValueError, match='scale_denom'):
            codec.jpeg_batch_layout([data], scale_denom=bad)
        with pytest.raises(ValueError, match='scale_denom'):
            codec.jpeg_render_dev(info, 0, 0, render='libjpeg', scale_denom=bad)
        with pytest.raises(ValueError, match='scale_denom'):
            codec.jpeg_scaled_size(9, 9, bad)
    for call in (lambda: codec.host_jpeg_render(*d, render='reference', scale_denom=2),
                 lambda: codec.host_jpeg_batch([data], scale_denom=2),
                 lambda: codec.jpeg_to_rgb(data, scale_denom=2),
                 lambda: codec.jpeg_batch_to_rgb([data, data], render='reference', scale_denom=[1, 4]),
                 lambda: codec.jpeg_render_dev(info, 0, 0, render='reference', scale_denom=8)):
        with pytest.raises(ValueError, match="needs render='libjpeg'"):
            call()
    with pytest.raises(ValueError, match='2 scale_denom values for 1 images'):
        codec.host_jpeg_batch([data], render='libjpeg', scale_denom=[2, 2])
    # the C calls themselves: JDS_EINVAL naming the value, nothing written
    st = codec._jpeg_info_struct(*d[1:])
    cf = np.ascontiguousarray(d[0], np.int16)
    img = np.full((9, 9, 3), 0x5A, np.uint8)
    lib = _abi.lib()
    with pytest.raises(ValueError, match='scale_denom 3 is not 1, 2, 4 or 8'):
        _abi.check(lib.jds_selftest_jpeg_render_scaled(C.byref(st), cf.ctypes.data, img.ctypes.data, 1, 3))
    with pytest.raises(ValueError, match='scale_denom 2 needs JDS_RENDER_LIBJPEG'):
        _abi.check(lib.jds_selftest_jpeg_render_scaled(C.byref(st), cf.ctypes.data, img.ctypes.data, 0, 2))
    with pytest.raises(ValueError, match='scale_denom 5'):
        _abi.check(lib.jds_jpeg_scaled_size(9, 9, 5, C.byref(C.c_int64()), C.byref(C.c_int64())))
    assert np.all(img == 0x5A)


def test_denominator_one_is_the_existing_call():
    import inspect
    from jds import codec
    from test_jpeg_render_cpu import host_render, mixed_batch as full_batch
    for f in (codec.jpeg_to_rgb, codec.jpeg_batch_to_rgb, codec.jpeg_batch_layout, codec.jpeg_render_dev,
              codec.host_jpeg_render, codec.host_jpeg_batch):
        assert inspect.signature(f).parameters['scale_denom'].default == 1
    for data in (pillow_file(33, 35, '4:2:0'), pillow_file(17, 23, '4:2:2'), pillow_file(9, 9, '4:4:4'),
                 pillow_file(37, 53, 'L')):
        for render in ('libjpeg', 'reference'):
            assert np.array_equal(codec.host_jpeg_render(*_decoded(data), render=render, scale_denom=1),
                                  host_render(data, render))
    files = full_batch()
    for render in ('libjpeg', 'reference'):
        a = codec.host_jpeg_batch(files, render=render)
        b = codec.host_jpeg_batch(files, render=render, scale_denom=1)
        c = codec.host_jpeg_batch(files, render=render, scale_denom=[1] * len(files))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert np.array_equal(a[0], c[0]) and a[2] == c[2]
    assert codec.jpeg_batch_layout(files) == codec.jpeg_batch_layout(files, scale_denom=1)


def test_draft_denom_is_pillows_choice():
    from PIL import Image
    from jds import codec
    sides = (1, 7, 8, 9, 16, 31, 64, 100)
    asks = (1, 2, 3, 5, 8, 13, 50, 200)
    for h in sides:
        for w in sides:
            buf = io.BytesIO()
            Image.new('L', (w, h)).save(buf, 'JPEG')
            for rh in asks:
                for rw in asks:
                    im = Image.open(io.BytesIO(buf.getvalue()))
                    im.draft('L', (rw, rh))
                    scale = im.decoderconfig[0] if im.decoderconfig else 1
                    assert codec.draft_denom(h, w, (rw, rh)) == scale, (h, w, rw, rh)
                    assert im.size == codec.jpeg_scaled_size(h, w, scale)[::-1]


def test_scaled_size():
    from jds import codec
    for h, w in [(1, 1), (7, 9), (8, 8), (1080, 1920), (1081, 1921)]:
        for d in (1, 2, 4, 8):
            assert codec.jpeg_scaled_size(h, w, d) == (-(-h // d), -(-w // d))
    assert codec.jpeg_scaled_size(1080, 1920, 8) == (135, 240)


def test_new_symbols_and_header():
    from jds import _abi
    lib = _abi.lib()
    names = ('jds_jpeg_scaled_size', 'jds_jpeg_render_scaled_dev', 'jds_jpeg_to_rgb_scaled',
             'jds_jpeg_batch_layout_scaled', 'jds_jpeg_batch_to_rgb_scaled', 'jds_selftest_jpeg_render_scaled',
             'jds_selftest_jpeg_batch_render_scaled')
    with open(os.path.join(ROOT, 'include', 'jds.h')) as f:
        h = f.read()
    for name in names:
        assert hasattr(lib, name) and f'int {name}(' in h, name
    assert 'no scaling' not in h


# --------------------------------------------------- 5. sanitizer program --

def test_tile_core_clean_under_host_sanitizers(tmp_path):
    """tools/jpeg_ljs_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: the host tile loop against a plain whole-plane implementation
    over every size up to 40 x 40 in the four modes at the three denominators, exactly-sized heap
    arrays, full-range coefficients with tables of 255 among them, and a mixed batch."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'jpeg_ljs_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'jpeg_ljs_san.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stderr == '', r.stderr[-4000:]
    images, checks, failed = (int(r.stdout.split()[i]) for i in (0, 2, 4))
    assert images > 3 * 6400 and checks > images and failed == 0
