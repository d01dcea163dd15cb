"""GPU checks of the scaled libjpeg rendering (k_jpeg_ljs, k_jpeg_ljs_batch; DESIGN.md "Scaled
libjpeg rendering"): jpeg_to_rgb / jpeg_batch_to_rgb with render='libjpeg' and scale_denom against
Pillow's Image.draft byte for byte, the launch alone against the host tile core between guard
bytes, a batch with mixed denominators, full-range coefficients, and decode-at-1/4 -> encode
against Pillow's thumbnail file.  Small sizes only: every tile path, no large image."""
import io

import numpy as np
import pytest

from test_jpeg_batch_cpu import flipped
from test_jpeg_interleaved_cpu import fixture
from test_jpeg_render_cpu import _decoded, hostile, pillow_file, pillow_pixels, tile_sizes
from test_jpeg_scale_cpu import DENOMS, MODES, draft_pixels

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 17), (17, 23), (31, 45), (40, 72), (16, 130), (130, 16)]
SMALL = [(1, 1), (3, 5), (5, 130)]                           # a side below (some) denominator


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def host_scaled(data, d):
    from jds import codec
    return codec.host_jpeg_render(*_decoded(data), render='libjpeg', scale_denom=d)


@pytest.mark.parametrize('mode', MODES)
def test_gpu_scaled_render_equals_pillow_draft(mode):
    from jds import codec
    for h, w in SIZES + tile_sizes() + SMALL:
        for q, kind in ((90, 'picture'), (100, 'noise')):
            data = pillow_file(h, w, mode, q, kind)
            for d in DENOMS:
                got = codec.jpeg_to_rgb(data, render='libjpeg', scale_denom=d)
                assert got.dtype == np.uint8 and got.shape == (-(-h // d), -(-w // d), 3)
                exp = draft_pixels(data, d) if h >= d and w >= d else host_scaled(data, d)
                assert np.array_equal(got, exp), (h, w, mode, q, d)


def test_gpu_scaled_render_to_a_device_tensor():
    import torch
    from jds import codec
    for mode in MODES:
        data = pillow_file(33, 129, mode)
        for d in DENOMS:
            oh, ow = codec.jpeg_scaled_size(33, 129, d)
            out = torch.full((oh, ow, 3), 0x5A, dtype=torch.uint8, device='cuda')
            got, info = codec.jpeg_to_rgb(data, out=out, render='libjpeg', scale_denom=d, with_info=True)
            assert got is out and (info['scale_denom'], info['out_H'], info['out_W']) == (d, oh, ow)
            assert (info['H'], info['W']) == (33, 129)
            assert np.array_equal(out.cpu().numpy(), draft_pixels(data, d)), (mode, d)
    full = torch.empty((33, 129, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match=r'\(17, 65, 3\)'):
        codec.jpeg_to_rgb(pillow_file(33, 129, '4:2:0'), out=full, render='libjpeg', scale_denom=2)


@pytest.mark.parametrize('lead', [64, 67])
def test_gpu_scaled_render_dev_equals_host_core_and_writes_only_the_image(lead):
    """jpeg_render_dev with scale_denom on decode_jpeg's coefficients, on torch tensors and torch's
    stream, between guard bytes.  The rows of 65 x 257 at 1/2, 1/4, 1/8 are 387, 195 and 99 bytes,
    so the row starts take every alignment and both the dword and the byte stores run; the two
    leads shift which rows take which."""
    import torch
    from jds import codec, entropy
    for mode in MODES:
        data = pillow_file(65, 257, mode)
        dd = entropy.decode_jpeg(data)
        coeffs = torch.from_numpy(dd['coeffs']).cuda()
        for d in DENOMS:
            oh, ow = codec.jpeg_scaled_size(dd['H'], dd['W'], d)
            n = oh * ow * 3
            buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device='cuda')
            codec.jpeg_render_dev(dd, coeffs.data_ptr(), buf.data_ptr() + lead, render='libjpeg', scale_denom=d,
                                  stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
            got = buf.cpu().numpy()
            assert np.all(got[:lead] == 0xA5) and np.all(got[lead + n:] == 0xA5), (mode, d)
            exp = codec.host_jpeg_render(dd['coeffs'], dd['H'], dd['W'], dd['mode'], dd['qtables'], dd['grids'],
                                         render='libjpeg', scale_denom=d)
            assert np.array_equal(got[lead:lead + n].reshape(oh, ow, 3), exp), (mode, d)


def batch_files():
    """(files, denominators): thirteen files -- the four modes, a restart file, tile-edge sizes,
    every denominator and 1, a file the parser rejects (index 3) and one with a defective scan
    (index 6)."""
    files = [pillow_file(31, 45, '4:2:0'), pillow_file(9, 9, '4:4:4'), pillow_file(37, 53, 'L'),
             b'\xff\xd8\xff\xe0\x00\x02not a jpeg', pillow_file(33, 129, '4:2:2'), fixture('p40x72_420_rst2')[0],
             flipped(fixture('p24x40_420')[0]), pillow_file(3, 4, '4:2:0'), pillow_file(65, 257, '4:2:0', 30),
             pillow_file(65, 257, '4:4:4', 100, 'noise'), pillow_file(33, 129, '4:2:2'), pillow_file(31, 45, '4:2:0'),
             pillow_file(65, 257, '4:2:0', 30)]
    return files, [2, 4, 8, 2, 2, 8, 4, 8, 4, 2, 1, 1, 8]


def test_gpu_scaled_batch():
    import torch
    from jds import codec
    files, dens = batch_files()
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files, scale_denom=dens)
    buf = torch.full((rgb_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    views, info = codec.jpeg_batch_to_rgb(files, out=buf, render='libjpeg', errors='return', with_info=True,
                                          scale_denom=dens)
    assert info['rgb_bytes'] == rgb_bytes
    got = buf.cpu().numpy()
    covered = np.zeros(rgb_bytes, bool)
    for i, (f, d, it, lay, v) in enumerate(zip(files, dens, info['items'], items, views)):
        assert it['scale_denom'] == d and it['rgb_off'] == lay['rgb_off']
        if i == 3:
            assert v is None and it['rc'] != 0 and it['rgb_off'] == -1
            continue
        oh, ow = codec.jpeg_scaled_size(it['H'], it['W'], d)
        assert (it['out_H'], it['out_W']) == (oh, ow) and it['rgb_off'] % 256 == 0
        o, n = it['rgb_off'], oh * ow * 3
        covered[o:o + n] = True
        if i == 6:
            assert v is None and it['rc'] == 0 and it['status'] != 0 and not got[o:o + n].any()
            continue
        assert it['status'] == 0 and v.device.type == 'cuda' and tuple(v.shape) == (oh, ow, 3)
        img = got[o:o + n].reshape(oh, ow, 3)
        single = codec.jpeg_to_rgb(f, render='libjpeg', scale_denom=d)
        assert np.array_equal(img, single), i
        pil = pillow_pixels(f) if d == 1 else draft_pixels(f, d) if min(it['H'], it['W']) >= d else host_scaled(f, d)
        assert np.array_equal(img, pil), i
    assert np.all(got[~covered] == 0xA5) and not covered.all()
    own = codec.jpeg_batch_to_rgb(files, out='device', render='libjpeg', errors='return', scale_denom=dens)
    for i, (v, w) in enumerate(zip(own, views)):
        assert (v is None and w is None) if i in (3, 6) else bool((v == w).all()), i
    host = codec.jpeg_batch_to_rgb(files, render='libjpeg', errors='return', scale_denom=dens)
    for i, (v, w) in enumerate(zip(host, views)):
        assert (v is None) if i in (3, 6) else np.array_equal(v, w.cpu().numpy()), i
    with pytest.raises(ValueError, match='^file 3: '):
        codec.jpeg_batch_to_rgb(files, render='libjpeg', scale_denom=dens)
    one = codec.jpeg_batch_to_rgb(files[:3], render='libjpeg', scale_denom=4)       # one denominator for all
    for f, v in zip(files[:3], one):
        assert np.array_equal(v, codec.jpeg_to_rgb(f, render='libjpeg', scale_denom=4))


@pytest.mark.parametrize('mode', ['4:4:4', '4:2:2', '4:2:0', 'gray'])
def test_gpu_scaled_hostile_coefficients_equal_the_host_core(mode):
    import torch
    from jds import codec
    th, tw = codec.jpeg_inverse_info()
    for seed, (h, w) in enumerate([(9, 9), (th + 1, tw + 1)]):
        cf, h, w, mode, q, grids = hostile(h, w, mode, seed)
        coeffs = torch.from_numpy(cf).cuda()
        for d in DENOMS:
            exp = codec.host_jpeg_render(cf, h, w, mode, q, grids, render='libjpeg', scale_denom=d)
            out = torch.full(exp.shape, 0x5A, dtype=torch.uint8, device='cuda')
            codec.jpeg_render_dev({'H': h, 'W': w, 'mode': mode, 'qtables': q, 'grids': grids}, coeffs.data_ptr(),
                                  out.data_ptr(), render='libjpeg', scale_denom=d,
                                  stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(out.cpu().numpy(), exp), (h, w, d)


def test_gpu_thumbnail_file_equals_pillows():
    """Decode at 1/4 to a device tensor, encode from it: the file Pillow writes from its draft."""
    import torch
    from PIL import Image
    from jds import codec
    data = pillow_file(64, 96, '4:2:0')
    thumb = torch.empty((16, 24, 3), dtype=torch.uint8, device='cuda')
    codec.jpeg_to_rgb(data, out=thumb, render='libjpeg', scale_denom=4)
    got = codec.rgb_to_jpeg(thumb, quality=80)
    im = Image.open(io.BytesIO(data))
    im.draft('RGB', (24, 16))
    assert im.size == (24, 16)
    buf = io.BytesIO()
    im.convert('RGB').save(buf, 'JPEG', quality=80, subsampling=2)
    assert bytes(got) == buf.getvalue()
