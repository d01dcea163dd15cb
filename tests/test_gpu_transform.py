"""GPU checks of the lossless transforms (csrc/jds_xform.hip: k_coef_xform between the batch
decode and the interleaved-scan writer, behind jds_jpeg_transform and jds_jpeg_batch_transform).
The yardsticks are the definition (tests/transform_ref.py), the host model, and Pillow (libjpeg)
wherever a round trip must give Pillow's own file back."""
import io

import numpy as np
import pytest
from PIL import Image

import transcode_cases as tc
import transform_cases as xc
import transform_ref as xr
from test_jpeg_batch_cpu import flipped

pytestmark = pytest.mark.gpu

CASES = xc.SIZES + [xc.MEDIUM]
CASE_IDS = [f'{h}x{w}-{m}' for h, w, m, _ in CASES]


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def dev(data, op, optimize=True, trim=False):
    from jds import codec
    return codec.jpeg_transform(data, op, trim=trim, optimize=optimize)


# ------------------------------------------------------- 7. the kernel alone --

@pytest.mark.parametrize('h,w,mode,ops', CASES, ids=CASE_IDS)
def test_gpu_coef_transform_against_numpy(h, w, mode, ops):
    """k_coef_xform on random int16 coefficients, -32768 and 32767 among them, against the
    NumPy coefficient transform: every block, every entry, every sign."""
    from jds import entropy
    cf, info = xc.extreme_coeffs(h, w, mode, 7 * h + w)
    assert cf.min() == -32768 and cf.max() == 32767
    if (h, w, mode) == xc.MEDIUM[:3]:
        assert [r * c for r, c in info['grids']] == [884, 221, 221] and 884 % 32 and 884 > 32
    for op in ops:
        want, oh, ow = xr.coef_transform(cf, h, w, mode, op)
        got = entropy.coef_transform_dev(cf, info, op)
        assert got.shape == want.shape and np.array_equal(got, want), op
    # with trim: the partial MCU column / row is dropped, every operation the mode allows
    if h % 16 or w % 16:
        for op in xc.allowed(h, w, mode, trim=True):
            want, oh, ow = xr.coef_transform(cf, h, w, mode, op, trim=True)
            got = entropy.coef_transform_dev(cf, info, op, trim=True)
            assert got.shape == want.shape and np.array_equal(got, want), (op, 'trim')


# ---------------------------------------- 8. against the reference, host model --

@pytest.mark.parametrize('optimize', [False, True])
@pytest.mark.parametrize('h,w,mode,ops', CASES, ids=CASE_IDS)
def test_gpu_transform_against_reference_and_host_model(h, w, mode, ops, optimize):
    from jds import codec, entropy
    src = tc.pillow(h, w, mode, 50, False, True)
    for op in ops:
        got = dev(src, op, optimize)
        assert got == xr.transform(src, op, False, optimize), op
        assert got == entropy.host_transform_jpeg(src, op, optimize=optimize), op
    assert dev(src, 'none', optimize) == codec.jpeg_transcode(src, optimize=optimize)


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_transform_foreign_files(optimize):
    for case in (tc.FOREIGN_CASES[1], tc.FOREIGN_CASES[4], tc.FOREIGN_CASES[7]):   # three tables; restart; three scans
        src = tc.foreign(*case)
        h, w, mode = case[:3]
        for trim in (False, True):
            for op in xc.allowed(h, w, mode, trim):
                assert dev(src, op, optimize, trim) == xr.transform(src, op, trim, optimize), (case, op, trim)


def test_gpu_transform_refusals_and_info():
    from jds import codec
    f = tc.pillow(37, 53, '4:2:0', 50, False, True)
    with pytest.raises(ValueError, match='width 53 is not a multiple of 16'):
        dev(f, 'hflip')
    got, info = codec.jpeg_transform(f, 'hflip', trim=True, with_info=True)
    assert got == xr.transform(f, 'hflip', True, True)
    assert (info['H'], info['W']) == (37, 53) and info['transform'] == {'op': 'hflip', 'H': 37, 'W': 48}
    with pytest.raises(ValueError, match='4:2:2 takes only'):
        dev(tc.pillow(32, 48, '4:2:2', 50, False, True), 'rot90')
    with pytest.raises(ValueError, match='trim leaves nothing'):
        dev(tc.pillow(7, 200, '4:2:0', 50, False, False), 'vflip', trim=True)
    with pytest.raises(ValueError, match='defective scan'):
        dev(flipped(tc.pillow(48, 80, '4:2:0', 50, False, False)), 'rot90')


# --------------------------------------------------------------- 9. round trips --

@pytest.mark.parametrize('h,w', [(48, 80), (208, 272)])
def test_gpu_round_trips_give_pillows_file_back(h, w):
    src = tc.pillow(h, w, '4:2:0', 50, True, True)
    f = src
    for i in range(4):
        f = dev(f, 'rot90')
        assert (f == src) == (i == 3)
    assert dev(dev(src, 'hflip'), 'hflip') == src
    assert dev(dev(src, 'transverse'), 'transverse') == src


# -------------------------------------------------------------- 10. mixed batch --

def mixed_batch():
    b = io.BytesIO()
    Image.fromarray(tc.image(24, 24)).save(b, 'JPEG', progressive=True)
    files = [(tc.pillow(1, 1, '4:4:4', 50, False, True), 'none'),
             (tc.pillow(208, 272, '4:2:0', 50, False, True), 'rot90'),
             (tc.pillow(32, 48, '4:2:2', 92, True, False), 'rot180'),
             (xc.quadrant_file(xc.exif_block(6, False)), 'auto'),
             (tc.pillow(37, 53, '4:2:0', 50, False, True), 'hflip'),           # 4: refused, no trim
             (b.getvalue(), 'rot90'),                                          # 5: the parser rejects it
             (flipped(tc.pillow(48, 80, '4:2:0', 50, False, False)), 'vflip'),  # 6: a corrupted scan
             (tc.foreign(*tc.FOREIGN_CASES[1]), 'transpose')]
    return [f for f, _ in files], [o for _, o in files], [0, 1, 2, 3, 7], 4, 5, 6


@pytest.mark.parametrize('optimize', [False, True])
def test_gpu_mixed_batch(optimize):
    import torch
    from jds import _abi, codec
    files, ops, good, refused, rejected, corrupt = mixed_batch()
    outs, items = codec.jpeg_batch_transform(files, ops, optimize=optimize, errors='items')
    assert [i for i, o in enumerate(outs) if o is not None] == good
    assert items[refused]['rc'] == _abi.JDS_ENOTSUP and items[rejected]['rc'] != 0
    for i in (refused, rejected):
        assert items[i]['out_len'] == 0 and items[i]['out_off'] == -1
    assert items[corrupt]['rc'] == 0 and items[corrupt]['status'] != 0
    assert items[corrupt]['out_len'] == 0 and items[corrupt]['out_off'] == -1
    off = 0
    for i in good:
        assert items[i]['out_off'] == off and off % 256 == 0 and items[i]['out_len'] == len(outs[i])
        off = -(-(off + len(outs[i])) // 256) * 256
    for i in good:
        assert outs[i] == dev(files[i], ops[i], optimize), i                  # the single call
        assert outs[i] == xr.transform(files[i], ops[i], False, optimize), i
    assert (items[1]['H'], items[1]['W']) == (272, 208) and (items[3]['H'], items[3]['W']) == (80, 48)
    assert Image.open(io.BytesIO(outs[3])).getexif()[0x0112] == 1
    with pytest.raises(ValueError, match=rf'file {refused}: .*width 53 is not a multiple of 16'):
        codec.jpeg_batch_transform(files, ops, optimize=optimize)
    # reordered: no good file's bytes change
    order = [7, 6, 3, 5, 1, 4, 0, 2]
    outs_r, items_r = codec.jpeg_batch_transform([files[i] for i in order], [ops[i] for i in order],
                                                 optimize=optimize, errors='items')
    assert outs_r == [outs[i] for i in order]
    # on the device, into a pre-filled buffer: the same bytes, the gaps untouched
    buf = torch.full((off + 512,), 0xA5, dtype=torch.uint8, device='cuda:0')
    views, items_d = codec.jpeg_batch_transform(files, ops, optimize=optimize, out=buf, errors='items')
    assert items_d == items
    host = buf.cpu().numpy()
    end = 0
    for i in good:
        o, n = items[i]['out_off'], items[i]['out_len']
        assert np.all(host[end:o] == 0xA5)
        assert host[o:o + n].tobytes() == outs[i] == views[i].cpu().numpy().tobytes()
        end = o + n
    assert np.all(host[end:] == 0xA5)
    views2, _ = codec.jpeg_batch_transform(files, ops, optimize=optimize, out='device', errors='items')
    assert [None if v is None else v.cpu().numpy().tobytes() for v in views2] == outs
    # one operation for all, and the plain transcode beside it
    allnone, _ = codec.jpeg_batch_transform(files, 'none', optimize=optimize, errors='items')
    plain, _ = codec.jpeg_batch_transcode(files, optimize=optimize, errors='items')
    assert allnone == plain


def test_gpu_empty_batch_and_argument_errors():
    from jds import codec
    assert codec.jpeg_batch_transform([]) == []
    assert codec.jpeg_batch_transform([], out='device', errors='items') == ([], [])
    f = tc.pillow(16, 16, '4:2:0', 50, False, True)
    with pytest.raises(ValueError, match='operations for'):
        codec.jpeg_batch_transform([f, f], ['hflip'])
    with pytest.raises(ValueError, match='unknown transform operation'):
        codec.jpeg_batch_transform([f], ['flop'])


# -------------------------------------------------------------- 11. full size --

def test_gpu_full_size_rot90_round_trip():
    """1088 x 1920 at 4:2:0 (68 x 120 whole MCUs, 765 writer segments: the long-scan route) on a
    transformed geometry: rot90 gives a 1920 x 1088 file, rot270 gives Pillow's file back."""
    from jds import entropy
    src = tc.pillow(1088, 1920, '4:2:0', 50, True, False)
    rot = dev(src, 'rot90')
    d = entropy.parse_jpeg(rot)
    assert (d['H'], d['W']) == (1920, 1088) and d['mcu']['rows'] * d['mcu']['cols'] * 6 == 48960
    assert dev(rot, 'rot270') == src
