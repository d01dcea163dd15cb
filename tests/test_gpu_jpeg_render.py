"""GPU checks of the libjpeg rendering (k_jpeg_ljt, k_jpeg_ljt_batch; DESIGN.md "libjpeg
rendering"): jpeg_to_rgb / jpeg_batch_to_rgb with render='libjpeg' against Pillow byte for byte,
the launch alone against the host tile core, full-range coefficients, and the default rendering
pinned from this side.  Small sizes only: every tile path, no large image."""
import numpy as np
import pytest

from oracle import cpu_ref
from test_jpeg_batch_cpu import flipped
from test_jpeg_interleaved_cpu import Q50, fixture
from test_jpeg_render_cpu import hostile, pillow_file, pillow_pixels, tile_sizes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def render_cases():
    """A subset of the CPU test's sizes across the three modes and gray, then the tile-edge sizes
    in every mode."""
    small = [(1, 1, '4:2:0'), (1, 1, '4:4:4'), (3, 4, '4:2:2'), (3, 4, '4:2:0'), (4, 5, '4:2:0'), (4, 5, '4:2:2'),
             (8, 8, '4:4:4'), (9, 9, '4:2:0'), (17, 23, '4:2:2'), (31, 45, '4:2:0'), (33, 35, '4:4:4'),
             (40, 72, '4:2:0'), (5, 130, '4:2:2'), (5, 130, '4:2:0'), (130, 6, '4:2:0'), (130, 6, '4:2:2'),
             (1, 1, 'L'), (7, 9, 'L'), (37, 53, 'L'), (5, 130, 'L')]
    return small + [(h, w, m) for h, w in tile_sizes() for m in ('4:4:4', '4:2:2', '4:2:0', 'L')]


def test_gpu_render_equals_pillow():
    from jds import codec
    for h, w, mode in render_cases():
        for q, kind in ((90, 'picture'), (100, 'noise')):
            data = pillow_file(h, w, mode, q, kind)
            got = codec.jpeg_to_rgb(data, render='libjpeg')
            assert got.dtype == np.uint8 and np.array_equal(got, pillow_pixels(data)), (h, w, mode, q)


def test_gpu_render_own_three_scan_file():
    """One of this library's own files (three non-interleaved scans) at a size whose grids are
    T.81's, which Pillow reads too."""
    from jds import codec, entropy
    h, w, mode = 64, 96, '4:2:0'
    raw = codec.compress_reconstruct_raw(cpu_ref.random_image(h, w, 3), 50, Q50, mode, True, maps=False)
    data = entropy.encode_jfif(raw['coeffs'], h, w, mode, Q50)[0]
    assert not entropy.parse_jpeg(data)['interleaved']
    assert np.array_equal(codec.jpeg_to_rgb(data, render='libjpeg'), pillow_pixels(data))


def test_gpu_render_to_a_device_tensor():
    import torch
    from jds import codec
    for mode in ('4:2:0', '4:2:2', '4:4:4', 'L'):
        data = pillow_file(33, 129, mode)
        out = torch.full((33, 129, 3), 0x5A, dtype=torch.uint8, device='cuda')
        assert codec.jpeg_to_rgb(data, out=out, render='libjpeg') is out
        assert np.array_equal(out.cpu().numpy(), pillow_pixels(data)), mode


@pytest.mark.parametrize('lead', [64, 67])
def test_gpu_render_dev_equals_host_core_and_writes_only_the_image(lead):
    """jpeg_render_dev on decode_jpeg's coefficients, on torch tensors and torch's stream, between
    guard bytes; lead = 67 puts the image at an odd address (the byte-store path)."""
    import torch
    from jds import codec, entropy
    for mode in ('4:2:0', '4:2:2', '4:4:4', 'L'):
        data = pillow_file(65, 257, mode)
        d = entropy.decode_jpeg(data)
        h, w, n = d['H'], d['W'], d['H'] * d['W'] * 3
        coeffs = torch.from_numpy(d['coeffs']).cuda()
        buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        codec.jpeg_render_dev(d, coeffs.data_ptr(), buf.data_ptr() + lead, render='libjpeg',
                              stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[:lead] == 0xA5) and np.all(got[lead + n:] == 0xA5)
        exp = codec.host_jpeg_render(d['coeffs'], h, w, d['mode'], d['qtables'], d['grids'], render='libjpeg')
        assert np.array_equal(got[lead:lead + n].reshape(h, w, 3), exp), mode
        buf.fill_(0xA5)                                      # render='reference' is jpeg_inverse_dev's launch
        codec.jpeg_render_dev(d, coeffs.data_ptr(), buf.data_ptr() + lead, render='reference',
                              stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(buf.cpu().numpy()[lead:lead + n].reshape(h, w, 3), codec.jpeg_to_rgb(data)), mode


def batch_files():
    """Ten files: the four modes, a restart file, an optimised-table file, tile-edge sizes, and one
    file with a defective scan (index 5)."""
    return [pillow_file(31, 45, '4:2:0'), pillow_file(9, 9, '4:4:4'), pillow_file(37, 53, 'L'),
            pillow_file(33, 129, '4:2:2'), fixture('p40x72_420_rst2')[0], flipped(fixture('p24x40_420')[0]),
            fixture('p31x45_420_q95_opt')[0], pillow_file(3, 4, '4:2:0'), pillow_file(65, 257, '4:2:0', 30),
            pillow_file(65, 257, '4:4:4', 100, 'noise')]


def test_gpu_batch_render():
    import torch
    from jds import codec
    files = batch_files()
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    buf = torch.full((rgb_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    views, info = codec.jpeg_batch_to_rgb(files, out=buf, render='libjpeg', errors='return', with_info=True)
    got = buf.cpu().numpy()
    covered = np.zeros(rgb_bytes, bool)
    for i, (f, it, v) in enumerate(zip(files, info['items'], views)):
        o, n = it['rgb_off'], it['H'] * it['W'] * 3
        covered[o:o + n] = True
        if i == 5:
            assert v is None and it['rc'] == 0 and it['status'] != 0 and not got[o:o + n].any()
            continue
        assert it['status'] == 0 and v.device.type == 'cuda'
        assert np.array_equal(got[o:o + n].reshape(it['H'], it['W'], 3), pillow_pixels(f)), i
    assert np.all(got[~covered] == 0xA5) and not covered.all()
    own = codec.jpeg_batch_to_rgb(files, out='device', render='libjpeg', errors='return')
    for i, (f, v) in enumerate(zip(files, own)):
        assert (v is None) if i == 5 else np.array_equal(v.cpu().numpy(), pillow_pixels(f)), i
    with pytest.raises(ValueError, match='^file 5: defective scan data'):
        codec.jpeg_batch_to_rgb(files, render='libjpeg')
    # the other rendering from this side: the same call with render='reference' is today's call --
    # the sentinel buffer byte for byte (images, the zeros of the defective one, the fill between)
    buf.fill_(0xA5)
    codec.jpeg_batch_to_rgb(files, out=buf, render='reference', errors='return')
    ref_buf = buf.cpu().numpy()
    buf.fill_(0xA5)
    codec.jpeg_batch_to_rgb(files, out=buf, errors='return')
    assert np.array_equal(ref_buf, buf.cpu().numpy()) and np.all(ref_buf[~covered] == 0xA5)
    assert not np.array_equal(ref_buf, got)                 # and it is the other rendering
    dev_ref = codec.jpeg_batch_to_rgb(files, out='device', render='reference', errors='return')
    dev_today = codec.jpeg_batch_to_rgb(files, out='device', errors='return')
    for i, (a, b) in enumerate(zip(dev_ref, dev_today)):
        assert (a is None and b is None) if i == 5 else bool((a == b).all()), i
    today = codec.jpeg_batch_to_rgb(files, errors='return')
    ref = codec.jpeg_batch_to_rgb(files, errors='return', render='reference')
    for i, (a, b, f) in enumerate(zip(today, ref, files)):
        if i == 5:
            assert a is None and b is None
            continue
        assert np.array_equal(a, b) and np.array_equal(a, codec.jpeg_to_rgb(f)), i
        assert np.array_equal(codec.jpeg_to_rgb(f, render='reference'), a), i


@pytest.mark.parametrize('mode', ['4:4:4', '4:2:2', '4:2:0', 'gray'])
def test_gpu_hostile_coefficients_equal_the_host_core(mode):
    import torch
    from jds import codec
    th, tw = codec.jpeg_inverse_info()
    for seed, (h, w) in enumerate([(9, 9), (31, 45), (th + 1, tw + 1)]):
        cf, h, w, mode, q, grids = hostile(h, w, mode, seed)
        exp = codec.host_jpeg_render(cf, h, w, mode, q, grids, render='libjpeg')
        coeffs = torch.from_numpy(cf).cuda()
        out = torch.full((h, w, 3), 0x5A, dtype=torch.uint8, device='cuda')
        codec.jpeg_render_dev({'H': h, 'W': w, 'mode': mode, 'qtables': q, 'grids': grids}, coeffs.data_ptr(),
                              out.data_ptr(), render='libjpeg', stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(out.cpu().numpy(), exp), (h, w)
