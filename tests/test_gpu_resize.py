"""GPU checks of Pillow resizing (k_resize, k_resize_batch; DESIGN.md "Pillow resizing"):
rgb_resize, rgb_batch_resize and jpeg_batch_to_tensor against Pillow's Image.resize (after
Image.draft for files) byte for byte, the launches between guard bytes at odd alignments, a ragged
decoded batch, and files that fail inside a batch.  Small sizes only: every tile path, the
tile-width shrink, both pass-through cases and the tall rule; no large image."""
import io

import numpy as np
import pytest

import pillow_resize_ref as pr
from test_jpeg_render_cpu import pillow_file
from test_resize_cpu import FILTERS, image, pillow, pillow_draft_resize, tile_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def device_cases(flt):
    """The tile-edge shapes, the upscale 23 x 17 -> 64 x 48, a reduction beyond 8-fold on both
    axes, pass-through on either axis, the tall rule on both sides of its threshold and a box
    whose first byte is at an odd offset."""
    c = [(h, w, 'noise', size, box) for h, w, size, box in tile_cases()]
    c += [(200, 300, 'noise', (31, 19), None),               # 9.7- and 10.5-fold
          (40, 40, 'checker', (27, 23), None), (30, 40, 'noise', (40, 11), None), (30, 40, 'noise', (13, 30), None),
          (30, 40, 'noise', (40, 30), None), (400, 4, 'noise', (7, 5), None), (401, 4, 'noise', (7, 5), None),
          (401, 4, 'noise', (3, 40), (0.5, 10, 3.5, 390.25)), (97, 150, 'noise', (20, 30), (7, 3, 120, 90))]
    return c


@pytest.mark.parametrize('flt', FILTERS)
def test_gpu_rgb_resize_equals_pillow(flt):
    import torch
    from jds import codec
    for h, w, kind, size, box in device_cases(flt):
        img = image(h, w, kind)
        exp = pillow(img, size, flt, box)
        got = codec.rgb_resize(torch.from_numpy(img.copy()).cuda(), size, pr.NAMES[flt], box)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == exp.shape
        assert np.array_equal(got.cpu().numpy(), exp), (flt, h, w, kind, size, box)
    img = image(97, 150)                                      # an array in, an array out
    got = codec.rgb_resize(img, (65, 17), flt)
    assert isinstance(got, np.ndarray) and np.array_equal(got, pillow(img, (65, 17), flt))


@pytest.mark.parametrize('lead', [64, 67])
def test_gpu_rgb_resize_writes_only_its_output_and_reads_at_any_alignment(lead):
    """Source and output inside 0xA5-filled buffers: with the lead of 67 both start at an odd
    address, and rows of 3 * 65 and 3 * 17 bytes take every alignment, so the word and the byte
    paths of the staging and of the stores both run.  Nothing outside the output changes."""
    import torch
    from jds import codec
    for flt in FILTERS:
        for h, w, size, box in [(97, 150, (65, 17), None), (97, 150, (17, 33), (1, 2, 140.5, 95)),
                                (401, 4, (7, 5), None), (30, 40, (40, 30), None)]:
            img = image(h, w)
            n_in, n_out = img.size, size[0] * size[1] * 3
            src = torch.full((lead + n_in + 64,), 0xA5, dtype=torch.uint8, device='cuda')
            src[lead:lead + n_in] = torch.from_numpy(img.reshape(-1).copy()).cuda()
            before = src.clone()
            buf = torch.full((lead + n_out + 64,), 0xA5, dtype=torch.uint8, device='cuda')
            out = buf[lead:lead + n_out].view(size[1], size[0], 3)
            ret = codec.rgb_resize(src[lead:lead + n_in].view(h, w, 3), size, flt, box, out=out)
            assert ret is out
            got = buf.cpu().numpy()
            assert np.all(got[:lead] == 0xA5) and np.all(got[lead + n_out:] == 0xA5), (flt, h, w, size)
            assert np.array_equal(got[lead:lead + n_out].reshape(size[1], size[0], 3), pillow(img, size, flt, box)), \
                (flt, h, w, size, box)
            assert torch.equal(src, before)


def ragged_files():
    """Six files of mixed sizes and modes."""
    return [pillow_file(31, 45, '4:2:0'), pillow_file(9, 9, '4:4:4'), pillow_file(37, 53, 'L'),
            pillow_file(33, 129, '4:2:2'), pillow_file(65, 257, '4:2:0', 30), pillow_file(130, 16, '4:4:4')]


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


@pytest.mark.parametrize('flt', [pr.BICUBIC, pr.LANCZOS, pr.BOX])
def test_gpu_batch_resize_over_a_ragged_decoded_batch(flt):
    import torch
    from jds import codec
    files, size = ragged_files(), (20, 18)
    imgs = codec.jpeg_batch_to_rgb(files, out='device', render='libjpeg')
    lead = 67
    n = len(files) * size[0] * size[1] * 3
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    out = buf[lead:lead + n].view(len(files), size[1], size[0], 3)
    got = codec.rgb_batch_resize(imgs, size, flt, out=out)
    assert got is out
    torch.cuda.current_stream().synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:lead] == 0xA5) and np.all(host[lead + n:] == 0xA5)
    res = host[lead:lead + n].reshape(len(files), size[1], size[0], 3)
    for i, f in enumerate(files):
        assert np.array_equal(res[i], pillow(pillow_rgb(f), size, flt)), (flt, i)
        assert np.array_equal(res[i], codec.rgb_resize(imgs[i], size, flt).cpu().numpy()), (flt, i)
    # separate allocations are gathered; one box for all, and a 4-D tensor
    own = [im.clone() for im in imgs]
    box = (1, 2, 8.5, 9)
    got = codec.rgb_batch_resize(own, size, flt, boxes=box).cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(got[i], pillow(pillow_rgb(f), size, flt, box)), (flt, i)
    stack = torch.from_numpy(np.stack([image(23, 17), image(23, 17, 'checker')])).cuda()
    got = codec.rgb_batch_resize(stack, (64, 48), flt, boxes=[None, (0, 0, 17, 11.5)]).cpu().numpy()
    assert np.array_equal(got[0], pillow(image(23, 17), (64, 48), flt))
    assert np.array_equal(got[1], pillow(image(23, 17, 'checker'), (64, 48), flt, (0, 0, 17, 11.5)))
    assert tuple(codec.rgb_batch_resize([], size, flt).shape) == (0, size[1], size[0], 3)


def test_gpu_batch_resize_with_tall_images():
    import torch
    from jds import codec
    imgs = [image(401, 4), image(30, 40), image(600, 5, 'checker'), image(400, 4)]
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    for flt in FILTERS:
        got = codec.rgb_batch_resize(dev, (7, 5), flt).cpu().numpy()
        for i, a in enumerate(imgs):
            assert np.array_equal(got[i], pillow(a, (7, 5), flt)), (flt, i)


@pytest.mark.parametrize('flt', FILTERS)
def test_gpu_jpeg_batch_to_tensor_equals_pillow_draft_resize(flt):
    import torch
    from jds import codec
    files = ragged_files() + [pillow_file(97, 130, '4:2:0'), pillow_file(130, 150, 'L')]
    size = (16, 16)
    exp = np.stack([pillow_draft_resize(f, size, flt) for f in files])
    got, info = codec.jpeg_batch_to_tensor(files, size, flt, with_info=True)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == exp.shape
    assert np.array_equal(got.cpu().numpy(), exp)
    assert [it['scale_denom'] for it in info['items']] == [codec.draft_denom(it['H'], it['W'], size)
                                                           for it in info['items']]
    assert {it['scale_denom'] for it in info['items']} == {1, 2, 4, 8} and info['rounds'] >= 0
    assert all((it['out_H'], it['out_W']) == codec.jpeg_scaled_size(it['H'], it['W'], it['scale_denom'])
               for it in info['items'])
    host = codec.jpeg_batch_to_tensor(files, size, flt, out=None)
    assert isinstance(host, np.ndarray) and np.array_equal(host, exp)
    lead = 67
    buf = torch.full((lead + exp.size + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    mine = buf[lead:lead + exp.size].view(*exp.shape)
    assert codec.jpeg_batch_to_tensor(files, size, pr.NAMES[flt], out=mine) is mine
    b = buf.cpu().numpy()
    assert np.all(b[:lead] == 0xA5) and np.all(b[lead + exp.size:] == 0xA5)
    assert np.array_equal(b[lead:lead + exp.size].reshape(exp.shape), exp)


def test_gpu_jpeg_batch_to_tensor_denominators_and_boxes():
    from PIL import Image
    from jds import codec
    files = ragged_files()
    dens = [1, 1, 2, 4, 8, 2]
    size, flt = (13, 11), pr.BICUBIC
    boxes = [(0.5, 1, 6.25, 7)] * len(files)

    def expect(f, d, box):
        im = Image.open(io.BytesIO(f))
        w, h = im.size
        if d > 1:
            im.draft('RGB', (w // d, h // d))
            assert im.decoderconfig[0] == d
        return np.asarray(im.convert('RGB').resize(size, flt, box))
    got = codec.jpeg_batch_to_tensor(files, size, 'bicubic', scale_denom=dens, out=None)
    for i, (f, d) in enumerate(zip(files, dens)):
        assert np.array_equal(got[i], expect(f, d, None)), i
    got = codec.jpeg_batch_to_tensor(files, size, 3, scale_denom=dens, boxes=boxes, out=None)
    for i, (f, d, b) in enumerate(zip(files, dens, boxes)):
        assert np.array_equal(got[i], expect(f, d, b)), i
    got = codec.jpeg_batch_to_tensor(files, size, 'bicubic', scale_denom=1, out=None)
    for i, f in enumerate(files):
        assert np.array_equal(got[i], expect(f, 1, None)), i
    with pytest.raises(ValueError, match='image 1: box .* not within the 9 x 9 image'):
        codec.jpeg_batch_to_tensor(files, size, 'bicubic', scale_denom=dens, boxes=[(0, 0, 8, 20)] * len(files))


def progressive_file():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image(40, 56)).save(buf, 'JPEG', progressive=True)
    return buf.getvalue()


def test_gpu_jpeg_batch_to_tensor_failed_files_keep_zeroed_slots():
    from jds import codec
    good = ragged_files()
    cut = pillow_file(65, 257, '4:2:0', 30)
    files = good[:2] + [cut[:len(cut) // 2], good[2], progressive_file()] + good[3:]
    size, flt = (16, 16), pr.LANCZOS
    got, idx, info = codec.jpeg_batch_to_tensor(files, size, flt, out=None, errors='return', with_info=True)
    assert idx == [2, 4]
    assert info['items'][4]['rc'] != 0
    for i in idx:
        assert not got[i].any(), i
    for i in range(len(files)):
        if i not in idx:
            assert np.array_equal(got[i], pillow_draft_resize(files[i], size, flt)), i
    with pytest.raises(ValueError, match=f'file {idx[0]}'):
        codec.jpeg_batch_to_tensor(files, size, flt)
    only_bad = codec.jpeg_batch_to_tensor([progressive_file(), b'nothing'], size, flt, out=None, errors='return')
    assert only_bad[1] == [0, 1] and not only_bad[0].any()
