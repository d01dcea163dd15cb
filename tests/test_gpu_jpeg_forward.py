"""GPU checks of the libjpeg encoding (k_jpeg_fwd, k_jpeg_fwd_batch; DESIGN.md "libjpeg
encoding"): the launch alone against the host tile core between guard regions, rgb_to_jpeg against
Pillow's bytes, a mixed batch with a bad item, and decode -> re-encode on the device against
Pillow's own re-save.  Small sizes only: every tile path (three tile rows and columns), no large
image."""
import io

import numpy as np
import pytest

from test_jpeg_forward_cpu import image, of_mode, pillow_save

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (17, 33), (33, 130), (70, 300)]             # the last: three tile rows, three tile columns
MODES = ['4:4:4', '4:2:2', '4:2:0', 'gray']


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared images are read-only)


@pytest.mark.parametrize('lead', [64, 67])
def test_gpu_forward_dev_equals_host_core_and_writes_only_the_coefficients(lead):
    """rgb_forward_dev on torch tensors and torch's stream: the image at byte `lead` of a larger
    buffer (67: an odd address, every row start misaligned), the coefficients between guards."""
    import torch
    from jds import codec
    guard = 64                                               # entries: the planes stay 16-byte aligned
    for h, w in SIZES:
        for mode in MODES:
            img = of_mode(image(h, w, 'noise', lead), mode)
            exp, info = codec.host_rgb_forward(img, 75, mode)
            src = torch.full((lead + img.size + 61,), 0xA5, dtype=torch.uint8, device='cuda')
            src[lead:lead + img.size] = to_dev(img).reshape(-1)
            cf = torch.full((guard + exp.size + guard,), 0x5A5A, dtype=torch.int16, device='cuda')
            codec.rgb_forward_dev(info, src.data_ptr() + lead, cf.data_ptr() + 2 * guard,
                                  stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
            got = cf.cpu().numpy()
            assert np.all(got[:guard] == 0x5A5A) and np.all(got[guard + exp.size:] == 0x5A5A), (h, w, mode)
            assert np.array_equal(got[guard:guard + exp.size], exp), (h, w, mode)


def test_gpu_forward_dev_refuses_a_misaligned_plane():
    import torch
    from jds import codec
    _, info = codec.host_rgb_forward(np.zeros((8, 8, 3), np.uint8))
    src = torch.zeros(192, dtype=torch.uint8, device='cuda')
    cf = torch.zeros(256, dtype=torch.int16, device='cuda')
    with pytest.raises(ValueError, match='16-byte aligned'):
        codec.rgb_forward_dev(info, src.data_ptr(), cf.data_ptr() + 2)


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_rgb_to_jpeg_equals_pillow(optimize):
    import torch
    from jds import codec
    for h, w in SIZES:
        for mode in MODES:
            for q in (10, 75, 95):
                img = of_mode(image(h, w, 'two-level' if q == 95 else 'noise', q), mode)
                exp = pillow_save(img, mode, q, optimize)
                assert codec.rgb_to_jpeg(img, q, mode, optimize) == exp, (h, w, mode, q)
                dev = to_dev(img)
                assert codec.rgb_to_jpeg(dev, q, mode, optimize) == exp, (h, w, mode, q)


def test_gpu_rgb_to_jpeg_arguments():
    import torch
    from jds import codec
    dev = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        codec.rgb_to_jpeg(dev[:, ::2])
    with pytest.raises(ValueError, match='uint8'):
        codec.rgb_to_jpeg(dev.to(torch.int16))
    with pytest.raises(ValueError, match='quality'):
        codec.rgb_to_jpeg(dev, quality=0)
    with pytest.raises(ValueError, match='HxWx3'):
        codec.rgb_to_jpeg(dev.reshape(16, 12, 4))


def mixed_batch():
    """Twelve images: every mode, the sizes above, two qualities, two identical items (4 and 9),
    and item 6 with quality 0."""
    shapes = [(17, 33, '4:2:0'), (1, 1, '4:4:4'), (33, 130, '4:2:2'), (70, 300, 'gray'), (33, 130, '4:2:0'),
              (70, 300, '4:4:4'), (17, 33, '4:2:2'), (1, 1, 'gray'), (70, 300, '4:2:0'), (33, 130, '4:2:0'),
              (17, 33, '4:4:4'), (1, 1, '4:2:2')]
    imgs = [of_mode(image(h, w, 'noise', 4 if i == 9 else i), m) for i, (h, w, m) in enumerate(shapes)]
    quals = [60 if i % 2 else 85 for i in range(12)]
    quals[9] = quals[4]
    quals[6] = 0
    return imgs, quals, [m for _, _, m in shapes]


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_batch_mixed(optimize):
    from jds import codec
    imgs, quals, modes = mixed_batch()
    assert np.array_equal(imgs[4], imgs[9])
    outs, items = codec.rgb_batch_to_jpeg(imgs, quals, modes, optimize, errors='items')
    assert len(outs) == 12 and outs[6] is None and items[6]['rc'] != 0 and items[6]['out_off'] == -1
    for i in range(12):
        if i != 6:
            assert items[i]['rc'] == 0 and outs[i] == codec.rgb_to_jpeg(imgs[i], quals[i], modes[i], optimize), i
    assert outs[4] == outs[9]
    assert outs[0] == pillow_save(imgs[0], modes[0], quals[0], optimize)
    with pytest.raises(ValueError, match='image 6: quality 0'):
        codec.rgb_batch_to_jpeg(imgs, quals, modes, optimize)
    keep = [i for i in range(12) if i != 6]                  # the neighbours do not depend on the bad item
    rest = codec.rgb_batch_to_jpeg([imgs[i] for i in keep], [quals[i] for i in keep], [modes[i] for i in keep], optimize)
    assert rest == [outs[i] for i in keep]


def test_gpu_batch_device_outputs_and_inputs():
    import torch
    from jds import codec
    imgs, quals, modes = mixed_batch()
    host = codec.rgb_batch_to_jpeg(imgs, quals, modes, errors='items')[0]
    dev_imgs = [to_dev(a) for a in imgs]      # separate allocations: gathered
    outs, items = codec.rgb_batch_to_jpeg(dev_imgs, quals, modes, out='device', errors='items')
    base = min(o.data_ptr() for o in outs if o is not None)
    for i, o in enumerate(outs):
        if i == 6:
            assert o is None
            continue
        assert o.is_cuda and (o.data_ptr() - base) % 256 == 0 and items[i]['out_off'] % 256 == 0
        assert o.cpu().numpy().tobytes() == host[i], i
    # views into one allocation, at odd offsets, are passed by offset
    pool = torch.full((3 * 33 * 130 * 3 + 200,), 0xA5, dtype=torch.uint8, device='cuda')
    views, o = [], 67
    for k in range(3):
        a = image(33, 130, 'noise', k)
        v = pool[o:o + a.size].view(33, 130, 3)
        v.copy_(to_dev(a))
        views.append(v)
        o += a.size + 1
    got = codec.rgb_batch_to_jpeg(views, 75, '4:2:0')
    assert got == [pillow_save(image(33, 130, 'noise', k), '4:2:0', 75) for k in range(3)]
    # an N x H x W x 3 tensor
    stack = torch.stack([to_dev(image(17, 33, 'noise', k)) for k in range(3)])
    got = codec.rgb_batch_to_jpeg(stack, [10, 75, 95], '4:2:2', optimize=True)
    assert got == [pillow_save(image(17, 33, 'noise', k), '4:2:2', q, True) for k, q in enumerate((10, 75, 95))]
    # a caller's buffer: too small names the need, large enough is used
    small = torch.zeros(256, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='output buffer too small'):
        codec.rgb_batch_to_jpeg(views, 75, '4:2:0', out=small)
    big = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    got = codec.rgb_batch_to_jpeg(views, 75, '4:2:0', out=big)
    assert all(g.data_ptr() >= big.data_ptr() and (g.data_ptr() - big.data_ptr()) % 256 == 0 for g in got)


def test_gpu_batch_empty():
    from jds import codec
    assert codec.rgb_batch_to_jpeg([]) == []
    assert codec.rgb_batch_to_jpeg([], out='device', errors='items') == ([], [])
    outs, items = codec.rgb_batch_to_jpeg([np.zeros((8, 8, 3), np.uint8)], quality=0, errors='items')
    assert outs == [None] and items[0]['rc'] != 0


def test_gpu_decode_then_encode_equals_pillow_resave():
    """jpeg_batch_to_rgb(out='device', render='libjpeg') feeds rgb_batch_to_jpeg: the bytes are
    Image.open(f).convert('RGB').save(quality=60)'s; a gray file rendered to (Y, Y, Y) is encoded
    as colour, as Pillow does after convert('RGB')."""
    from PIL import Image
    from jds import codec
    files, exp = [], []
    for h, w in ((50, 31), (64, 48)):
        for mode in MODES:
            f = pillow_save(of_mode(image(h, w, 'ramp'), mode), mode, 90)
            files.append(f)
            buf = io.BytesIO()
            Image.open(io.BytesIO(f)).convert('RGB').save(buf, 'JPEG', quality=60)
            exp.append(buf.getvalue())
    tensors = codec.jpeg_batch_to_rgb(files, out='device', render='libjpeg')
    got = codec.rgb_batch_to_jpeg(tensors, quality=60)
    assert got == exp
