"""CPU checks of grayscale (one-component) files (no GPU): the parser, the host decode model,
the host tile loop of the gray inverse, the host model of the batch, the writer's and the
transforms' host models, the rejections by name, and the stand-alone sanitizer program
(tools/jpeg_gray_san.cpp).  Expected coefficients: gray_ref.decode (T.81 F.2 in NumPy over the
file's DHT); expected pixels: gray_ref.oracle_image (the per-stage definition with the oracle's
stages); expected files: gray_ref.write / gray_ref.transform and Pillow's own files."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import gray_ref as g
import transform_ref as xr
from conftest import ROOT

OPS7 = ['hflip', 'vflip', 'transpose', 'transverse', 'rot90', 'rot180', 'rot270']


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def pillow_pixels(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == 'L'
    return np.asarray(im)


@pytest.mark.parametrize('name', sorted(g.FILES))
def test_parse_decode_and_render_on_the_host(name):
    from jds import codec, entropy
    data = g.file(name)
    r = g.decode(data)
    d = entropy.parse_jpeg(data)
    h, w, save = g.FILES[name]
    gr, gc = -(-h // 8), -(-w // 8)
    assert (d['H'], d['W'], d['mode'], d['components']) == (h, w, 'gray', 1)
    assert not d['interleaved'] and not d['reference_grid'] and d['single_table']
    assert d['grids'] == [(gr, gc), (0, 0), (0, 0)] and d['sampling'] == [(1, 1), (0, 0), (0, 0)]
    assert d['mcu'] == {'rows': gr, 'cols': gc, 'blocks': 1} and d['coeffs_needed'] == 64 * gr * gc
    assert d['qtables'].shape == (3, 8, 8) and np.array_equal(d['qtables'][0], r['qtable']) and not d['qtables'][1:].any()
    assert d['tq'] == [r['tq'], 0, 0] and len(d['scans']) == 1
    sc = d['scans'][0]
    assert sc['components'] == [1] and (sc['dc_tables'], sc['ac_tables']) == ([r['tables'][0]], [r['tables'][1]])
    assert sc['restart_interval'] == r['ri'] and data[sc['offset']:sc['offset'] + sc['length']] == r['segment']
    assert r['sampling'] == (0x22 if save.get('subsampling') == 2 else 0x11)
    if 'restart_marker_blocks' in save:
        assert r['ri'] == save['restart_marker_blocks']
    if 'restart_marker_rows' in save:
        assert r['ri'] == gc * save['restart_marker_rows']         # DRI counts blocks
    for (tc, th), (bits, vals) in r['huff'].items():
        assert d['huffman'][('dc', 'ac')[tc] + str(th)] == (bits, vals)
    for S in (64, 1024):
        cf, rounds = entropy.host_decode_jpeg(data, S)
        assert np.array_equal(cf, r['planar']) and len(rounds) == 1 and (rounds[0] == 0) == bool(r['ri'])
    exp = g.oracle_image(r['planar'], h, w, r['qtable'], r['grid'])
    got = codec.host_jpeg_inverse(r['planar'], h, w, 'gray', d['qtables'], d['grids'])
    assert got.shape == (h, w, 3) and np.array_equal(got, exp)
    assert np.abs(exp[:, :, 0].astype(int) - pillow_pixels(data)).max() <= 1     # a decode of this file


def test_sampling_byte_does_not_change_the_geometry():
    """Pillow's subsampling=2 writes 0x22 into a one-component SOF0: still 5 x 7 = 35 blocks and
    the same scan bytes as the 0x11 file."""
    from jds import entropy
    a, b = g.file('37x53'), g.file('37x53-0x22')
    assert len(a) == len(b) and g.decode(a)['segment'] == g.decode(b)['segment']
    da, db = entropy.parse_jpeg(a), entropy.parse_jpeg(b)
    assert da['grids'][0] == db['grids'][0] == (5, 7) and da['mcu'] == db['mcu']
    assert np.array_equal(entropy.host_decode_jpeg(a)[0], entropy.host_decode_jpeg(b)[0])
    sof = a.index(b'\xff\xc0')
    for smp in range(0x11, 0x45):
        if 1 <= smp >> 4 <= 4 and 1 <= smp & 15 <= 4:
            f = a[:sof + 11] + bytes([smp]) + a[sof + 12:]
            assert entropy.parse_jpeg(f)['grids'][0] == (5, 7), hex(smp)


def test_any_component_id():
    from jds import entropy
    a = g.file('9x9')
    sof, sos = a.index(b'\xff\xc0'), a.index(b'\xff\xda')
    for cid in (0, 1, 7, 255):
        f = a[:sof + 10] + bytes([cid]) + a[sof + 11:sos + 5] + bytes([cid]) + a[sos + 6:]
        d = entropy.parse_jpeg(f)
        assert d['mode'] == 'gray' and d['scans'][0]['components'] == [1]
        assert np.array_equal(entropy.host_decode_jpeg(f)[0], g.decode(a)['planar'])
        out = entropy.host_transcode_jpeg(f, True)
        assert out == g.transcode(f, True) and out[out.index(b'\xff\xda') + 5] == cid


def test_host_inverse_at_tile_edges_and_saturation():
    """Sizes around the 32 x 128 tile with coefficients that saturate both ends."""
    from jds import codec
    th, tw = codec.jpeg_inverse_info()
    rng = np.random.default_rng(3)
    q = rng.integers(1, 5, (8, 8)).astype(np.float64)
    for h, w in ((1, 1), (7, 9), (th - 1, tw + 1), (th + 1, 2 * tw - 1), (2 * th + 1, tw + 1)):
        gr, gc = -(-h // 8), -(-w // 8)
        cf = (rng.integers(-60, 61, (gr * gc, 64)) * (rng.random((gr * gc, 64)) < 0.9)).astype(np.int16).reshape(-1)
        info = g.info_of(h, w, q)
        got = codec.host_jpeg_inverse(cf, h, w, 'gray', info['qtables'], info['grids'])
        exp = g.oracle_image(cf, h, w, q, (gr, gc))
        assert np.array_equal(got, exp), (h, w)
        if h * w >= 64:    # both ends of the range and a large interior share: not an equality of clipped constants
            assert (exp == 0).any() and (exp == 255).any() and np.mean((exp > 0) & (exp < 255)) > 0.3


def test_inverse_argument_checks():
    import ctypes as C
    from jds import _abi, codec
    q = np.full((8, 8), 16.0)
    info = g.info_of(16, 24, q)
    cf = np.zeros(64 * 6, np.int16)
    bad = info['qtables'].copy()
    bad[0, 0, 5] = 0
    with pytest.raises(ValueError, match=r'qtable\[0\]\[5\]'):
        codec.host_jpeg_inverse(cf, 16, 24, 'gray', bad, info['grids'])
    junk = info['qtables'].copy()
    junk[1:] = -3.5                         # only component 0's table is checked
    assert codec.host_jpeg_inverse(cf, 16, 24, 'gray', junk, info['grids']).shape == (16, 24, 3)
    st = codec._jpeg_info_struct(16, 24, 'gray', info['qtables'], info['grids'])
    st.grid_cols[0] = 4
    with pytest.raises(ValueError, match='T.81 geometry'):
        _abi.check(_abi.lib().jds_jpeg_inverse_dev(None, C.byref(st), None, None, None))
    st = codec._jpeg_info_struct(16, 24, 'gray', info['qtables'], info['grids'])
    st.coeffs_needed = 3 * 64 * 6           # three planes' worth: one is what a gray file has
    with pytest.raises(ValueError, match='T.81 geometry'):
        _abi.check(_abi.lib().jds_jpeg_inverse_dev(None, C.byref(st), None, None, None))


def test_host_batch_mix():
    from jds import codec, entropy
    files = g.mix()
    rgb, cf, items = codec.host_jpeg_batch(files)
    lay, rb, ce = codec.jpeg_batch_layout(files)
    assert rb == rgb.size and ce == cf.size
    assert [it['mode'] for it in items] == ['gray', '4:2:0', 'gray', '4:4:4', 'gray', None]
    assert [it['rc'] == 0 for it in items] == [True] * 5 + [False]
    ro = co = 0
    for it, f in zip(items, files):
        if it['rc'] != 0:
            assert (it['rgb_off'], it['coef_off'], it['coeffs_needed']) == (-1, -1, 0)
            continue
        assert it['rgb_off'] % 256 == 0 and (it['rgb_off'], it['coef_off']) == (ro, co)
        n = it['H'] * it['W'] * 3
        end = it['rgb_off'] + n
        assert np.all(rgb[end:-(-end // 256) * 256] == 0xA5)
        img = rgb[it['rgb_off']:end].reshape(it['H'], it['W'], 3)
        if it['status']:
            assert not img.any()
        else:
            d = entropy.parse_jpeg(f)
            c1, _ = entropy.host_decode_jpeg(f)
            assert np.array_equal(cf[co:co + it['coeffs_needed']], c1)
            assert np.array_equal(img, codec.host_jpeg_inverse(c1, d['H'], d['W'], d['mode'], d['qtables'], d['grids']))
        ro += -(-n // 256) * 256
        co += it['coeffs_needed']
    assert items[4]['status'] != 0 and items[0]['status'] == items[2]['status'] == 0
    assert [it['mode'] for it in lay] == [it['mode'] for it in items]


@pytest.mark.parametrize('size', [(9, 9), (37, 53), (40, 136)])
def test_host_transcode_against_pillow(size):
    """Pillow's plain and optimize=True files of one picture are each other's transcodes, byte for
    byte; a restart file transcodes to the plain file; Pillow reads the outputs to the same pixels."""
    from jds import entropy
    h, w = size
    plain, opt = g.pillow_gray(h, w, 0), g.pillow_gray(h, w, 0, optimize=True)
    rst = g.pillow_gray(h, w, 0, restart_marker_blocks=2)
    assert plain != opt
    assert entropy.host_transcode_jpeg(opt, False) == plain == g.transcode(opt, False)
    assert entropy.host_transcode_jpeg(plain, True) == opt == g.transcode(plain, True)
    assert entropy.host_transcode_jpeg(rst, False) == plain
    assert entropy.host_transcode_jpeg(rst, True) == opt
    px = pillow_pixels(plain)
    for out in (entropy.host_transcode_jpeg(opt, False), entropy.host_transcode_jpeg(plain, True),
                entropy.host_transcode_jpeg(rst, True)):
        assert np.array_equal(pillow_pixels(out), px)
    assert entropy.host_transcode_jpeg(plain, True).count(b'\xff\xc4') == 2


def test_host_encode_extreme_coefficients():
    from jds import entropy
    h, w = 16, 24
    q = np.full((8, 8), 1.0)
    info = g.info_of(h, w, q)
    cf = g.extreme_coeffs(h, w)
    hist = g.histograms(cf)
    assert hist['dc0'][11] >= 2 and sum(hist['ac0'][(r << 4) | 10] for r in range(16)) >= 3 and hist['dc0'][0] >= 1
    for optimize in (False, True):
        out = entropy.host_encode_jpeg(cf, info, optimize)
        assert out == g.write(cf, g.default_prefix(h, w, q), optimize)
        d = entropy.parse_jpeg(out)
        assert d['mode'] == 'gray' and d['sampling'][0] == (1, 1) and np.array_equal(d['qtables'][0], q)
        assert np.array_equal(entropy.host_decode_jpeg(out)[0], cf) and np.array_equal(g.decode(out)['planar'], cf)
        assert np.array_equal(pillow_pixels(out).shape, (h, w))
        pfx = b'\xff\xfe\x00\x05abc' + g.default_prefix(h, w, q, tq=3)     # a caller's prefix, verbatim
        assert entropy.host_encode_jpeg(cf, info, optimize, prefix=pfx) == g.write(cf, pfx, optimize)
    for bad in (g.extreme_coeffs(h, w, dc_cat=12), g.extreme_coeffs(h, w, ac_cat=11)):
        with pytest.raises(ValueError, match='not baseline-codable'):
            entropy.host_encode_jpeg(bad, info, True)
    with pytest.raises(ValueError, match='coefficients'):
        entropy.host_encode_jpeg(np.zeros(3 * 64 * 6, np.int16), info)


@pytest.mark.parametrize('op', OPS7)
def test_host_transform_equals_the_block_reference(op):
    from jds import entropy
    data = g.pillow_gray(16, 24, 0)
    for optimize in (False, True):
        out = entropy.host_transform_jpeg(data, op, False, optimize)
        assert out == g.transform(data, op, False, optimize)
    d = entropy.parse_jpeg(out)
    assert (d['H'], d['W']) == ((24, 16) if op in xr.TRANSPOSING else (16, 24)) and d['mode'] == 'gray'
    # the pixels: Pillow's decode of the output is the same operation on Pillow's decode of the input
    # (whole blocks on both axes: every operation is exact)
    src = pillow_pixels(data)
    want = {'hflip': src[:, ::-1], 'vflip': src[::-1], 'transpose': src.T, 'transverse': src[::-1, ::-1].T,
            'rot90': src.T[:, ::-1], 'rot180': src[::-1, ::-1], 'rot270': src[:, ::-1].T}[op]
    assert np.abs(pillow_pixels(out).astype(int) - want).max() <= 1


@pytest.mark.parametrize('name', ['37x53', '37x53-0x22'])
def test_host_transform_trim_and_refusal(name):
    """The MCU of a one-component file is 8 x 8 whatever its sampling byte says."""
    from jds import codec, entropy
    data = g.file(name)
    with pytest.raises(ValueError, match=r'width 53 is not a multiple of 8'):
        entropy.host_transform_jpeg(data, 'hflip')
    out = entropy.host_transform_jpeg(data, 'hflip', True)
    assert out == g.transform(data, 'hflip', True) and entropy.parse_jpeg(out)['W'] == 48
    assert codec.jpeg_transform_info(data, 'hflip', True)['W'] == 48
    out = entropy.host_transform_jpeg(data, 'rot90', True)     # mirrors the source's vertical axis: 37 -> 32
    d = entropy.parse_jpeg(out)
    assert out == g.transform(data, 'rot90', True) and (d['H'], d['W']) == (53, 32)
    out = entropy.host_transform_jpeg(data, 'rot270', True)    # the horizontal one: 53 -> 48
    d = entropy.parse_jpeg(out)
    assert out == g.transform(data, 'rot270', True) and (d['H'], d['W']) == (48, 37)


def test_host_transform_rot90_trims_53_to_48():
    """rot90 mirrors the source's vertical axis (tests/transform_ref.py): on a file 53 rows high
    the trim takes 53 to 48 on that axis."""
    from jds import entropy
    data = g.pillow_gray(53, 37, 0)
    with pytest.raises(ValueError, match=r'height 53 is not a multiple of 8'):
        entropy.host_transform_jpeg(data, 'rot90')
    out = entropy.host_transform_jpeg(data, 'rot90', True)
    d = entropy.parse_jpeg(out)
    assert out == g.transform(data, 'rot90', True) and (d['H'], d['W']) == (37, 48)


def test_host_transform_auto_reads_and_resets_exif():
    from jds import codec, entropy
    data = g.with_exif_orientation(g.pillow_gray(16, 24, 0), 6)
    assert xr.exif_orientation(data[2:data.index(b'\xff\xdb')])[0] == 6
    assert codec.jpeg_transform_info(data, 'auto')['op'] == 'rot90'
    out = entropy.host_transform_jpeg(data, 'auto')
    assert out == g.transform(data, 'auto') == g.transform(g.with_exif_orientation(g.pillow_gray(16, 24, 0), 1), 'rot90')
    d = entropy.parse_jpeg(out)
    assert (d['H'], d['W']) == (24, 16)
    assert xr.exif_orientation(out[2:out.index(b'\xff\xdb')])[0] == 1
    assert entropy.host_transform_jpeg(out, 'auto') == entropy.host_transcode_jpeg(out, True)


def test_rejections_by_name():
    from jds import entropy
    a = g.file('9x9')
    sos = a.index(b'\xff\xda')
    three = g.with_sos(a, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    with pytest.raises(ValueError, match='grayscale'):
        entropy.parse_jpeg(three)
    second = a[:-2] + a[sos:]
    with pytest.raises(ValueError, match='second scan in a grayscale'):
        entropy.parse_jpeg(second)
    other = g.with_sos(a, bytes([1, 2, 0x00, 0, 63, 0]))
    with pytest.raises(ValueError, match='grayscale'):
        entropy.parse_jpeg(other)
    sof = a.index(b'\xff\xc0')
    for nf in (2, 4):
        f = a[:sof + 9] + bytes([nf]) + a[sof + 10:]
        with pytest.raises(ValueError, match=f'{nf} components'):
            entropy.parse_jpeg(f)
    with pytest.raises(ValueError, match='grayscale'):
        entropy.parse_jfif(a)                                   # this library's own profile only
    for smp in (0x01, 0x10, 0x51, 0x15):
        with pytest.raises(ValueError, match='sampling factors'):
            entropy.parse_jpeg(a[:sof + 11] + bytes([smp]) + a[sof + 12:])
    with pytest.raises(ValueError, match='progressive'):
        entropy.parse_jpeg(a[:sof + 1] + b'\xc2' + a[sof + 2:])


def test_abi_stays_3_and_the_struct_keeps_its_layout():
    import ctypes as C
    from jds import _abi
    assert _abi.lib().jds_abi_version() == 3
    assert _abi.SS_GRAY == 3 and _abi.JPEG_MODE_CODES['gray'] == 3 and 'gray' not in _abi.MODE_CODES
    with open(os.path.join(ROOT, 'include', 'jds.h')) as f:
        assert '#define JDS_SS_GRAY 3' in f.read()
    assert C.sizeof(_abi.JpegBatchItem) == 56


def test_gray_path_clean_under_host_sanitizers(tmp_path):
    """tools/jpeg_gray_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: parser, host decode, writer geometry, inverse arguments and host
    tile loop, default prefix, transform plan and prefix editor over one-component files of every
    sampling byte 0x11..0x44, every truncation of one, and hostile variants."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'jpeg_gray_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'jpeg_gray_san.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stderr == '', r.stderr[-4000:]
    files, checks, failed = (int(r.stdout.split()[i]) for i in (0, 2, 4))
    assert files == 6 * 16 and checks > 5000 and failed == 0
