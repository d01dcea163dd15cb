"""CPU checks of Pillow resizing (no GPU; DESIGN.md "Pillow resizing"): the NumPy definition
tests/pillow_resize_ref.py against the installed Pillow's Image.resize byte for byte, the
library's coefficient builder against the definition entry for entry, the kernel's tile core on
the host (jds_selftest_resize) against Pillow at the device's tile sizes, the 32-bit accumulator
bound of every table built, the refusals by name, the host model of jpeg_batch_to_tensor against
Pillow's draft + resize, and the stand-alone sanitizer program."""
import functools
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import pillow_resize_ref as pr
from conftest import ROOT

FILTERS = (pr.LANCZOS, pr.BILINEAR, pr.BICUBIC, pr.BOX, pr.HAMMING)


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


@functools.lru_cache(maxsize=None)
def image(h, w, kind='noise'):
    """noise: uniform bytes; checker: 0 / 255 squares of two pixels, which make bicubic and
    Lanczos overshoot on both sides of the range."""
    if kind == 'checker':
        y, x = np.mgrid[0:h, 0:w]
        a = np.repeat((((y // 2 + x // 2) & 1) * 255)[:, :, None], 3, 2)
        a[:, :, 1] = 255 - a[:, :, 1]
    else:
        a = np.random.default_rng([h, w]).integers(0, 256, (h, w, 3))
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


def pillow(img, size, flt, box=None):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize(size, flt, box))


def cases():
    """(h, w, kind, (width, height), box): up- and downscale, (1, 1) outputs, identity sizes with
    and without a box, integer and fractional boxes, the checker, 1 x N and N x 1 images, and the
    tall rule on either side of its threshold."""
    c = [(23, 17, 'noise', (48, 64), None), (48, 64, 'noise', (17, 23), None), (48, 64, 'noise', (1, 1), None),
         (5, 7, 'noise', (1, 1), None), (30, 40, 'noise', (40, 30), None), (30, 40, 'noise', (40, 30), (1, 2, 39, 29)),
         (30, 40, 'noise', (40, 30), (0, 0, 40, 29)), (30, 40, 'noise', (40, 11), None),
         (30, 40, 'noise', (13, 30), None), (45, 67, 'noise', (16, 16), (3, 5, 50, 41)),
         (45, 67, 'noise', (20, 9), (67 / 3, 45 / 4, 67 / 3 + 1.7, 45 / 4 + 2.2)),
         (45, 67, 'noise', (9, 20), (0.5, 0.25, 66.5, 44.75)), (40, 40, 'checker', (27, 23), None),
         (40, 40, 'checker', (64, 70), None), (40, 40, 'checker', (13, 40), None), (1, 37, 'noise', (11, 1), None),
         (1, 37, 'noise', (50, 3), None), (37, 1, 'noise', (1, 11), None), (37, 1, 'noise', (2, 50), None),
         (200, 300, 'noise', (7, 5), None), (400, 4, 'noise', (7, 5), None), (401, 4, 'noise', (7, 5), None),
         (401, 4, 'noise', (7, 401), None), (401, 4, 'noise', (3, 40), (0.5, 10, 3.5, 390.25)),
         (401, 4, 'checker', (5, 77), None)]
    return c


# ------------------------------------------- 1. the definition equals Pillow --

@pytest.mark.parametrize('flt', FILTERS)
def test_model_equals_pillow(flt):
    for h, w, kind, size, box in cases():
        img = image(h, w, kind)
        exp = pillow(img, size, flt, box)
        got = pr.resize(img, size, flt, box)
        assert got.shape == exp.shape == (size[1], size[0], 3)
        assert np.array_equal(got, exp), (flt, h, w, kind, size, box)


def test_checker_exercises_the_clamp_on_both_sides():
    """Before the clamp the 0 / 255 checker under- and overshoots with bicubic and Lanczos."""
    img = image(40, 40, 'checker').astype(np.int64)
    for flt in (pr.BICUBIC, pr.LANCZOS):
        K, B = pr.coeffs(40, 0, 40, 64, flt)
        s = np.stack([(1 << 21) + img[:, a:a + n, 0] @ K[xx, :n] for xx, (a, n) in enumerate(B)], 1) >> pr.PB
        assert s.min() < 0 and s.max() > 255


# ----------------------------------- 2. the library's tables equal the definition --

AXES = [(64, 0, 64, 17), (17, 0, 17, 64), (67, 67 / 3, 67 / 3 + 1.7, 20), (45, 0.25, 44.75, 20), (300, 0, 300, 7),
        (401, 10, 390.25, 40), (1, 0, 1, 5), (37, 0, 37, 1), (1080, 0, 1080, 224), (270, 0, 270, 224)]


@pytest.mark.parametrize('flt', FILTERS)
def test_library_coefficients_equal_the_definition(flt):
    from jds import codec
    for in_size, in0, in1, out_size in AXES:
        K, B = pr.coeffs(in_size, in0, in1, out_size, flt)
        ks, bounds, taps = codec.host_resize_coeffs(in_size, in0, in1, out_size, flt)
        assert ks == K.shape[1], (flt, in_size, out_size)
        assert np.array_equal(bounds, B) and np.array_equal(taps, K), (flt, in_size, in0, in1, out_size)


# ------------------------------- 3. the host tile loop equals Pillow at the tile's edges --

def tile_cases():
    """Output widths and heights tile - 1, tile, tile + 1 and 2 * tile + 3, and a horizontal
    reduction at which a 64-column segment no longer fits and the host shrinks the tile width."""
    from jds import codec
    th, tw, _ = codec.resize_info()
    c = [(97, 150, (w, h), None) for w, h in ((tw - 1, th - 1), (tw, th), (tw + 1, th + 1), (2 * tw + 3, 2 * th + 3))]
    c += [(200, 300, (tw + 1, th + 1), None), (97, 150, (tw + 1, 2 * th + 3), (2.5, 3, 140.25, 90)),
          (5, 45 * (tw + 1), (tw + 1, 3), None),        # 45-fold: 64 x 45 x 3 bytes and the support exceed the segment
          (23, 17, (64, 48), None)]
    return c


@pytest.mark.parametrize('flt', FILTERS)
def test_host_core_equals_pillow_at_tile_edges(flt):
    from jds import codec
    for h, w, size, box in tile_cases():
        img = image(h, w)
        got = codec.host_rgb_resize(img, size, flt, box)
        assert got.dtype == np.uint8 and np.array_equal(got, pillow(img, size, flt, box)), (flt, h, w, size, box)


@pytest.mark.parametrize('flt', FILTERS)
def test_host_core_equals_pillow_on_the_models_cases(flt):
    from jds import codec
    for h, w, kind, size, box in cases():
        img = image(h, w, kind)
        assert np.array_equal(codec.host_rgb_resize(img, size, pr.NAMES[flt], box), pillow(img, size, flt, box)), \
            (flt, h, w, kind, size, box)


def test_accumulator_bound_of_every_table_built(capsys):
    """255 * sum|k| + 2^21 of every table the cases above build fits in 31 bits; the largest is
    printed (DESIGN.md quotes it)."""
    from jds import codec
    worst, where = 0, None
    for flt in FILTERS:
        for h, w, kind, size, box in cases() + [(h, w, 'noise', s, b) for h, w, s, b in tile_cases()]:
            _, v = codec.host_rgb_resize(image(h, w, kind), size, flt, box, with_worst=True)
            if v > worst:
                worst, where = v, (pr.NAMES[flt], h, w, size, box)
    with capsys.disabled():
        print(f'\nlargest 255 * sum|k| + 2^21: {worst} = {worst / 2 ** 31:.4f} * 2^31 at {where}')
    assert 255 * (1 << 22) <= worst < (1 << 31)


# ------------------------------------------------------------- 4. refusals --

def test_refusals_by_name():
    import ctypes as C
    from jds import _abi, codec
    th, tw, max_taps = codec.resize_info()
    assert max_taps >= 512 and th >= 1 and tw >= 1
    img = image(9, 12)
    # bilinear needs 2 * ceil(scale) + 1 taps: scale (max_taps + 1) / 2 needs max_taps + 2
    n = (max_taps + 1) // 2
    wide = np.zeros((1, 2 * n, 3), np.uint8)
    with pytest.raises(ValueError, match=f'horizontal axis needs {max_taps + 2} taps per output sample.*cap is {max_taps}'):
        codec.host_rgb_resize(wide, (2, 1), 'bilinear')
    with pytest.raises(ValueError, match=f'vertical axis needs {max_taps + 2} taps'):
        codec.host_rgb_resize(wide.reshape(2 * n, 1, 3), (1, 2), 'bilinear')
    assert codec.host_rgb_resize(np.zeros((1, 2 * n - 2, 3), np.uint8), (2, 1), 'bilinear').shape == (1, 2, 3)   # the cap itself
    for bad in (0, 6, -1, 99):
        with pytest.raises(ValueError, match=f'unknown resampling filter {bad}'):
            codec.host_rgb_resize(img, (4, 4), bad)
    for bad in ('nearest', 'cubic', None, 2.0, True):
        with pytest.raises(ValueError, match='unknown resampling filter'):
            codec.host_rgb_resize(img, (4, 4), bad)
    for box in ((-1, 0, 12, 9), (0, 0, 12.5, 9), (0, 0, 12, 9.01), (5, 0, 5, 9), (6, 0, 5, 9), (0, 4, 12, 4),
                (0, 0, float('nan'), 9)):
        with pytest.raises(ValueError, match='box .* is empty or not within the 12 x 9 image'):
            codec.host_rgb_resize(img, (4, 4), 'bicubic', box)
        from PIL import Image
        if box[0] != box[2] and box[1] != box[3] and box[2] == box[2]:       # (an empty box Pillow lets through; NaN it rejects late)
            with pytest.raises(ValueError):
                Image.fromarray(img).resize((4, 4), 3, box)
    with pytest.raises(ValueError, match='box must be'):
        codec.host_rgb_resize(img, (4, 4), 'bicubic', (0, 0, 1))
    for size in ((0, 4), (4, 0), (-3, 4)):
        with pytest.raises(ValueError, match='bad size'):
            codec.host_rgb_resize(img, size, 'box')
    with pytest.raises(ValueError, match='size must be'):
        codec.host_rgb_resize(img, 4, 'box')
    with pytest.raises(ValueError, match='HxWx3'):
        codec.host_rgb_resize(img[:, :, 0], (4, 4), 'box')
    # the C calls themselves: nothing is written
    out = np.full((4, 4, 3), 0x5A, np.uint8)
    with pytest.raises(ValueError, match='unknown resampling filter 0'):
        _abi.check(_abi.lib().jds_selftest_resize(img.ctypes.data, 9, 12, None, 4, 4, 0, out.ctypes.data, None))
    assert np.all(out == 0x5A)
    with open(os.path.join(ROOT, 'include', 'jds.h')) as f:
        h = f.read()
    for name in ('jds_resize_info', 'jds_rgb_resize', 'jds_rgb_batch_resize', 'jds_jpeg_batch_to_tensor',
                 'jds_selftest_resize', 'jds_selftest_resize_coeffs'):
        assert hasattr(_abi.lib(), name) and f'int {name}(' in h, name
    assert C.sizeof(_abi.ResizeItem) == 48


# ------------------------------------- 5. jpeg_batch_to_tensor's host model --

def draft_files():
    """Four small Pillow files whose draft denominators for (16, 16) are 1, 2, 4 and 8."""
    from test_jpeg_render_cpu import pillow_file
    return [pillow_file(25, 31, '4:4:4'), pillow_file(45, 67, '4:2:2'), pillow_file(97, 130, '4:2:0'),
            pillow_file(130, 150, 'L')]


def pillow_draft_resize(data, size, flt, box=None):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft('RGB', size)
    return np.asarray(im.convert('RGB').resize(size, flt, box))


@pytest.mark.parametrize('flt', FILTERS)
def test_batch_to_tensor_host_model_equals_pillow_draft_resize(flt):
    from jds import codec
    files, size = draft_files(), (16, 16)
    lay, _, _ = codec.jpeg_batch_layout(files)
    dens = [codec.draft_denom(it['H'], it['W'], size) for it in lay]
    assert dens == [1, 2, 4, 8]
    rgb, _, items = codec.host_jpeg_batch(files, render='libjpeg', scale_denom=dens)
    for f, it in zip(files, items):
        o, n = it['rgb_off'], it['out_H'] * it['out_W'] * 3
        dec = np.ascontiguousarray(rgb[o:o + n].reshape(it['out_H'], it['out_W'], 3))
        assert np.array_equal(codec.host_rgb_resize(dec, size, flt), pillow_draft_resize(f, size, flt)), (flt, it)


# --------------------------------------------------- 6. sanitizer program --

def test_tile_core_clean_under_host_sanitizers(tmp_path):
    """tools/resize_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: the host tile loop against a plain whole-image two-pass
    implementation, every input size up to 24 x 24 to every output size up to 12 x 12 for the five
    filters, boxes, a tall image and 0 / 255 inputs, on exactly sized heap arrays."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'resize_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'resize_san.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stderr == '', r.stderr[-4000:]
    images, failed = (int(r.stdout.split()[i]) for i in (0, 2))
    assert images >= 5 * 24 * 24 * 12 * 12 and failed == 0
