"""GPU checks of grayscale (one-component) files through the writer and the transforms:
jpeg_transcode / jpeg_batch_transcode, encode_jpeg with mode 'gray', jpeg_transform /
jpeg_batch_transform against their host models (which tests/test_gray_cpu.py ties to the NumPy
definition and to Pillow's own files), alone and mixed with colour files in one batch, and the
luma-only histogram."""
import numpy as np
import pytest

import gray_ref as g

pytestmark = pytest.mark.gpu

OPS7 = ['hflip', 'vflip', 'transpose', 'transverse', 'rot90', 'rot180', 'rot270']


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_gray_transcode(optimize):
    from jds import codec, entropy
    names = ['1x1', '9x9', '37x53', '37x53-0x22', '40x136', '40x136-opt', '37x53-ri2', '40x136-rows1']
    for name in names:
        data = g.file(name)
        out, info = codec.jpeg_transcode(data, optimize, with_info=True)
        assert out == entropy.host_transcode_jpeg(data, optimize), name
        assert info['mode'] == 'gray' and info['components'] == 1
    assert codec.jpeg_transcode(g.file('40x136-opt'), False) == g.file('40x136')      # Pillow's own pair
    assert codec.jpeg_transcode(g.file('40x136'), True) == g.file('40x136-opt')
    big = g.long_file()                                                              # many segments, several rounds
    assert codec.jpeg_transcode(big, optimize) == entropy.host_transcode_jpeg(big, optimize)


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_gray_batch_transcode_mixed(optimize):
    """Gray and colour files in one set of writer launches; the defective and the unparseable
    file are item errors that change nobody else's bytes."""
    from jds import codec, entropy
    files = g.mix()
    outs, items = codec.jpeg_batch_transcode(files, optimize, errors='items')
    for k in range(4):
        assert bytes(outs[k]) == entropy.host_transcode_jpeg(files[k], optimize), k
        assert items[k]['rc'] == 0 and items[k]['status'] == 0 and items[k]['out_off'] % 256 == 0
    assert [it['mode'] for it in items] == ['gray', '4:2:0', 'gray', '4:4:4', 'gray', None]
    assert outs[4] is None and items[4]['rc'] == 0 and items[4]['status'] != 0
    assert outs[5] is None and items[5]['rc'] != 0
    gray_only = [g.file(n) for n in ('9x9', '37x53-opt', '40x136-rows1', '1x1')]
    for o, f in zip(codec.jpeg_batch_transcode(gray_only, optimize), gray_only):
        assert bytes(o) == entropy.host_transcode_jpeg(f, optimize)


def test_gpu_gray_histogram_counts_luma_only():
    from jds import entropy
    data = g.file('40x136')
    d = g.decode(data)
    got = entropy.transcode_histogram_dev(d['planar'], g.info_of(d['H'], d['W'], d['qtable']))
    want = g.histograms(d['planar'])
    assert np.array_equal(got['dc0'], want['dc0']) and np.array_equal(got['ac0'], want['ac0'])
    assert want['dc0'].sum() == 5 * 17 and not got['dc1'].any() and not got['ac1'].any()


def test_gpu_gray_encode_extreme_coefficients():
    from jds import entropy
    h, w = 16, 24
    q = np.full((8, 8), 1.0)
    info, cf = g.info_of(h, w, q), g.extreme_coeffs(h, w)
    for optimize in (False, True):
        out = entropy.encode_jpeg(cf, info, optimize)
        assert out == entropy.host_encode_jpeg(cf, info, optimize)
        assert np.array_equal(entropy.decode_jpeg(out)['coeffs'], cf)
        pfx = b'\xff\xfe\x00\x05abc' + g.default_prefix(h, w, q, tq=3)
        assert entropy.encode_jpeg(cf, info, optimize, prefix=pfx) == entropy.host_encode_jpeg(cf, info, optimize, prefix=pfx)
    for bad in (g.extreme_coeffs(h, w, dc_cat=12), g.extreme_coeffs(h, w, ac_cat=11)):
        with pytest.raises(ValueError, match='not baseline-codable'):
            entropy.encode_jpeg(bad, info, True)


@pytest.mark.parametrize('op', OPS7 + ['none'])
def test_gpu_gray_transform(op):
    from jds import codec, entropy
    data = g.pillow_gray(16, 24, 0)
    for optimize in (False, True):
        assert codec.jpeg_transform(data, op, False, optimize) == entropy.host_transform_jpeg(data, op, False, optimize)
    odd = g.file('40x136')                      # 5 x 17 blocks: several tiles of 32 destination blocks, a partial one
    assert codec.jpeg_transform(odd, op, True) == entropy.host_transform_jpeg(odd, op, True)


def test_gpu_gray_transform_trim_refusal_and_auto():
    from jds import codec, entropy
    for name in ('37x53', '37x53-0x22'):
        data = g.file(name)
        with pytest.raises(ValueError, match=r'width 53 is not a multiple of 8'):
            codec.jpeg_transform(data, 'hflip')
        out = codec.jpeg_transform(data, 'hflip', True)
        assert out == entropy.host_transform_jpeg(data, 'hflip', True) and entropy.parse_jpeg(out)['W'] == 48
        out = codec.jpeg_transform(data, 'rot90', True)
        assert out == entropy.host_transform_jpeg(data, 'rot90', True)
    tall = g.pillow_gray(53, 37, 0)
    out = codec.jpeg_transform(tall, 'rot90', True)        # 53 -> 48 on the mirrored axis
    d = entropy.parse_jpeg(out)
    assert out == entropy.host_transform_jpeg(tall, 'rot90', True) and (d['H'], d['W']) == (37, 48)
    ex = g.with_exif_orientation(g.pillow_gray(16, 24, 0), 6)
    out = codec.jpeg_transform(ex, 'auto')
    assert out == entropy.host_transform_jpeg(ex, 'auto') and entropy.parse_jpeg(out)['H'] == 24


def test_gpu_gray_batch_transform_mixed_with_colour():
    from jds import codec
    gray, colour = g.pillow_gray(16, 24, 0), g.pillow_colour(32, 48, 2)
    ex = g.with_exif_orientation(gray, 6)
    files = [gray, colour, g.file('37x53'), colour, ex, g.file('37x53-0x22')]
    ops = ['rot90', 'hflip', 'rot180', 'transpose', 'auto', 'hflip']
    outs, items = codec.jpeg_batch_transform(files, ops, trim=False, errors='items')
    for k in (0, 1, 3, 4):
        assert bytes(outs[k]) == codec.jpeg_transform(files[k], ops[k]), k
    assert outs[2] is None and items[2]['rc'] != 0        # 37 x 53: partial blocks on a mirrored axis, refused without trim
    assert outs[5] is None and items[5]['rc'] != 0
    outs = codec.jpeg_batch_transform(files, ops, trim=True)
    for k in range(6):
        assert bytes(outs[k]) == codec.jpeg_transform(files[k], ops[k], True), k
