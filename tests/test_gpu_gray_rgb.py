"""GPU checks of grayscale (one-component) files through decode and render: decode_jpeg and
jpeg_to_rgb against the NumPy reader (gray_ref.decode) and the per-stage definition
(gray_ref.oracle_image) at partial blocks and tiles, with the sampling byte 0x22, optimised
tables, both restart routes, more than one propagation round, output left on the device, the
staged route, the batch with colour files beside them, and a colour file before and after a
gray one in one Context."""
import numpy as np
import pytest

import gray_ref as g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def check_file(data, want_ri=None):
    from jds import codec, entropy
    r = g.decode(data)
    d = entropy.decode_jpeg(data)
    assert (d['mode'], d['components'], d['H'], d['W']) == ('gray', 1, r['H'], r['W'])
    assert d['grids'] == [r['grid'], (0, 0), (0, 0)] and d['coeffs_needed'] == r['planar'].size
    assert np.array_equal(d['coeffs'], r['planar']), f"rounds {d['rounds']}"
    assert np.array_equal(d['coeffs'], entropy.host_decode_jpeg(data)[0])
    if want_ri is not None:
        assert d['scans'][0]['restart_interval'] == want_ri
    img, info = codec.jpeg_to_rgb(data, with_info=True)
    exp = g.oracle_image(r['planar'], r['H'], r['W'], r['qtable'], r['grid'])
    assert img.dtype == np.uint8 and img.shape == (r['H'], r['W'], 3)
    assert np.array_equal(img, exp), np.argwhere(img != exp)[:4]
    assert info['route'] == 'fused' and np.array_equal(info['coeffs'], r['planar'])
    return d, img


@pytest.mark.parametrize('name', ['1x1', '9x9', '37x53', '37x53-0x22', '40x136', '37x53-opt'])
def test_gpu_gray_decode_and_render(name):
    """Partial blocks on both axes; 40x136: 2x2 tiles with a partial tile on each axis and the
    128-column boundary inside a row of blocks; 0x22: the sampling byte changes nothing."""
    d, img = check_file(g.file(name))
    assert d['rounds'] >= 1
    if name == '37x53-0x22':
        assert d['grids'][0] == (5, 7) and np.array_equal(img, check_file(g.file('37x53'))[1])


def test_gpu_gray_restart_routes():
    from jds import entropy
    lane_max = entropy.restart_info()[1]
    assert 17 <= lane_max
    d, _ = check_file(g.file('37x53-ri2'), 2)
    assert d['rounds'] == 0
    d, _ = check_file(g.file('40x136-rows1'), 17)          # one lane per interval
    assert d['rounds'] == 0
    h, w = 24, 8 * (lane_max + 3)                          # two full intervals beyond a lane's, one short row of blocks
    data = g.pillow_gray(h, w, 0, restart_marker_blocks=lane_max + 1)
    d, _ = check_file(data, lane_max + 1)                  # the descriptor route
    assert d['rounds'] >= 1


def test_gpu_gray_several_rounds():
    d, _ = check_file(g.long_file())
    assert d['rounds'] >= 2


def test_gpu_gray_output_on_the_device_and_staged_route():
    import torch
    from jds import codec
    data = g.file('40x136')
    host = codec.jpeg_to_rgb(data)
    out = torch.empty(host.shape, dtype=torch.uint8, device='cuda')
    assert codec.jpeg_to_rgb(data, out=out) is out
    assert np.array_equal(out.cpu().numpy(), host)
    img, info = codec.decompress_jpeg(data, with_info=True)
    assert info['route'] == 'staged' and np.array_equal(img, host)
    with pytest.raises(ValueError, match='plan route'):
        codec.decompress_jpeg(data, staged=False)
    # the plan route itself: JDS_ENOTSUP, as for any file the plan cannot take
    import ctypes as C
    from jds import _abi
    a = np.frombuffer(data, np.uint8)
    info, rgb = _abi.JpegInfo(), np.zeros(host.size, np.uint8)
    with _abi.lease(0) as ctx:
        rc = _abi.lib().jds_decompress_jpeg(ctx.handle, a.ctypes.data, a.size, rgb.ctypes.data, rgb.size, None,
                                            C.byref(info))
    assert rc == _abi.JDS_ENOTSUP and b'grayscale' in _abi.lib().jds_last_error() and not rgb.any()


def test_gpu_gray_inverse_dev_between_guards():
    """jpeg_inverse_dev on device coefficients: only the image's bytes are written."""
    import torch
    from jds import codec, entropy
    data = g.file('37x53')
    d = entropy.decode_jpeg(data)
    n = d['H'] * d['W'] * 3
    cf = torch.from_numpy(d['coeffs']).cuda()
    buf = torch.full((64 + n + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    codec.jpeg_inverse_dev(d, cf.data_ptr(), buf.data_ptr() + 64, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:64] == 0x5A) and np.all(got[64 + n:] == 0x5A)
    assert np.array_equal(got[64:64 + n].reshape(d['H'], d['W'], 3), codec.jpeg_to_rgb(data))


def test_gpu_gray_in_a_mixed_batch():
    import torch
    from jds import codec
    files = g.mix()
    singles, rounds = [], []
    for f in files[:4]:
        img, info = codec.jpeg_to_rgb(f, with_info=True)
        singles.append(img)
        rounds.append(info['rounds'])
    lay, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    out = torch.full((rgb_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    imgs, info = codec.jpeg_batch_to_rgb(files, out=out, with_info=True, errors='return')
    buf = out.cpu().numpy()
    items = info['items']
    assert [it['mode'] for it in items] == ['gray', '4:2:0', 'gray', '4:4:4', 'gray', None]
    for k in range(4):
        assert np.array_equal(imgs[k].cpu().numpy(), singles[k]), k
    bad = items[4]
    assert bad['rc'] == 0 and bad['status'] != 0 and imgs[4] is None
    o = bad['rgb_off']
    assert o % 256 == 0 and not buf[o:o + bad['H'] * bad['W'] * 3].any()
    assert items[5]['rc'] != 0 and imgs[5] is None
    for it in items[:5]:
        end = it['rgb_off'] + it['H'] * it['W'] * 3
        assert it['rgb_off'] % 256 == 0 and np.all(buf[end:-(-end // 256) * 256] == 0xA5)
    assert info['rounds'] == max(rounds)
    host = codec.jpeg_batch_to_rgb(files, errors='return')
    for k in range(4):
        assert np.array_equal(host[k], singles[k])
    with pytest.raises(ValueError, match='file 4'):
        codec.jpeg_batch_to_rgb(files[:5])


def test_gpu_colour_file_around_a_gray_one():
    """One Context: the shared scratch does not carry the one-component geometry over."""
    from jds import _abi, codec
    colour, gray = g.pillow_colour(37, 53, 2), g.file('40x136')
    before = codec.jpeg_to_rgb(colour)
    ctx = _abi.Context(0)
    try:
        a = codec.jpeg_batch_to_rgb([colour], ctx=ctx)[0]
        b = codec.jpeg_batch_to_rgb([gray], ctx=ctx)[0]
        c = codec.jpeg_batch_to_rgb([colour], ctx=ctx)[0]
    finally:
        ctx.close()
    assert np.array_equal(a, before) and np.array_equal(c, before)
    assert np.array_equal(b, codec.jpeg_to_rgb(gray))
    assert np.array_equal(codec.jpeg_to_rgb(colour), before)    # the pooled context, after gray files
