"""The certified fast inverse's per-block paths at the window's edges
(csrc/jds_inv_fast.hip: sign-extending column loads, the chroma window stores
at one base per task, the written-out plane / task / round loops).

Three things can go wrong there: the sign of a coefficient, the window columns
a ring block or a block at the image's edge writes, and which column a task or
round works on.  The in-kernel exact fallback would hide any of them by
recomputing the tile, so every case also pins fix_counts()[1] to what the
parent of that change reported for the same input (FIX, measured once on the
device; random frames of at most 16 tiles: none recomputed).

Bytes, coefficients and statistics are compared with
oracle.cpu_ref.compress_reconstruct; the negated-coefficient runs with the
oracle's inverse stages (the chain of tests/params_ref.py:60-70)."""
import numpy as np
import pytest

from oracle import cpu_ref
from test_gpu_inv_fast import _plan

pytestmark = pytest.mark.gpu

Q = 50
# heights: aligned tiles; raised tiles whose first tile row has no block row
# -1; raised tiles with a partial last tile row
HEIGHTS = (64, 120, 136)
# widths: both image edges in one tile (ke = 7); a second tile of two pixels
# (ke = 0 in its first interior block); ke = 3; 144; three tile columns, the
# last nearly empty; an odd width
WIDTHS = (128, 130, 136, 144, 264, 131)
MODES = (('4:2:0', True), ('4:2:0', False), ('4:2:2', False))
# tiles the parent commit's library recomputed per (mode, prefilter, h, w, way);
# absent: 0
FIX = {}


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def _img(h, w, mode, pf):
    return cpu_ref.random_image(h, w, 2100 + 7 * h + w + (100000 if mode == '4:2:2' else 0) + (50000 if pf else 0))


def inverse_ref(coeffs, q, mode, h, w, block=8):
    """The oracle's inverse stages on given coefficients (Y, Cb, Cr blocks in
    raster order): dequantise, IDCT, merge, crop, upsample, colour, clip."""
    qm = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)
    if block == 16:
        qm = cpu_ref.quant_table16(qm)
    ch, cw = (h // 2 if mode == '4:2:0' else h), (w if mode == '4:4:4' else w // 2)
    rec, off = [], 0
    for ph, pw in ((h, w), (ch, cw), (ch, cw)):
        padded = (-(-ph // block) * block, -(-pw // block) * block)
        n = padded[0] * padded[1]
        qb = coeffs[off:off + n].reshape(-1, block, block)
        off += n
        r = cpu_ref.decode_blocks(cpu_ref.dequantize(qb, qm))
        rec.append(cpu_ref.merge_blocks(r, padded)[:ph, :pw])
    assert off == coeffs.size
    y, cb, cr = rec
    if mode != '4:4:4':
        cb, cr = cpu_ref.upsample_chroma(cb, cr, (h, w))
    return np.clip(cpu_ref.ycbcr_to_rgb(np.stack([y, cb, cr], axis=-1)), 0, 255).astype(np.uint8)


def _check_stats(st, ref):
    assert [int(v) for v in st['hist']] == [int(v) for v in ref['hist']]
    assert int(st['nonzero']) == ref['bitrate']['nonzero_count']


def _fix(key, way, fix):
    print(f'fix_counts {key + (way,)}: {int(fix[1])}')
    assert int(fix[1]) == FIX.get(key + (way,), 0), (key, way, fix)


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('h', HEIGHTS)
@pytest.mark.parametrize('mode,pf', MODES)
def test_window_edges(mode, pf, h, w):
    from jds import _abi
    key = (mode, pf, h, w)
    img = _img(h, w, mode, pf)
    ref = cpu_ref.compress_reconstruct(img, Q, 8, mode, pf, metrics=False)
    frames = img[None]
    # a full run: the a-priori instantiation
    (out, cf, st, fix), = _plan(frames, [Q], mode, pf, [0])
    assert np.array_equal(cf[0], ref['coeffs'])
    assert np.array_equal(out[0], ref['reconstructed']), int(np.sum(out[0] != ref['reconstructed']))
    _check_stats(st[0], ref)
    _fix(key, 'full', fix)
    # inverse only, on the coefficients the forward wrote: the tracked instantiation
    (out2, cf2, st2, fix2), = _plan(frames, [Q], mode, pf, [0], coeffs=cf)
    assert np.array_equal(cf2, cf)
    assert np.array_equal(out2[0], ref['reconstructed']), int(np.sum(out2[0] != ref['reconstructed']))
    _fix(key, 'inv', fix2)
    # with the SSE terms (XTRA = 1)
    (out3, cf3, st3, fix3), = _plan(frames, [Q], mode, pf, [_abi.RUN_SSE])
    assert np.array_equal(cf3[0], ref['coeffs'])
    assert np.array_equal(out3[0], ref['reconstructed']), int(np.sum(out3[0] != ref['reconstructed']))
    _check_stats(st3[0], ref)
    d = img.astype(np.int64) - ref['reconstructed'].astype(np.int64)
    assert int(st3[0]['sse_rgb']) == int(np.sum(d * d))
    _fix(key, 'sse', fix3)
    # sign extension: the forward's coefficients negated (the same |q Q|,
    # mostly negative low frequencies), inverse only
    neg = (-cf.astype(np.int32)).astype(np.int16)
    (out4, cf4, st4, fix4), = _plan(frames, [Q], mode, pf, [0], coeffs=neg)
    want = inverse_ref(neg[0], Q, mode, h, w)
    assert np.array_equal(out4[0], want), int(np.sum(out4[0] != want))
    _fix(key, 'neg', fix4)


def test_window_edges_444():
    """k_inv_fast444 (its fix-up count is in waves of eight blocks)."""
    h, w, mode = 72, 136, '4:4:4'
    key = (mode, False, h, w)
    img = cpu_ref.random_image(h, w, 2301)
    ref = cpu_ref.compress_reconstruct(img, Q, 8, mode, False, metrics=False)
    (out, cf, st, fix), = _plan(img[None], [Q], mode, False, [0])
    assert np.array_equal(cf[0], ref['coeffs'])
    assert np.array_equal(out[0], ref['reconstructed'])
    _check_stats(st[0], ref)
    _fix(key, 'full', fix)
    (out2, cf2, st2, fix2), = _plan(img[None], [Q], mode, False, [0], coeffs=cf)
    assert np.array_equal(out2[0], ref['reconstructed'])
    _fix(key, 'inv', fix2)
    neg = (-cf.astype(np.int32)).astype(np.int16)
    (out4, cf4, st4, fix4), = _plan(img[None], [Q], mode, False, [0], coeffs=neg)
    assert np.array_equal(out4[0], inverse_ref(neg[0], Q, mode, h, w))
    _fix(key, 'neg', fix4)


def test_window_edges_block16():
    """k_inv16_fast: 16 x 16 blocks at 4:2:2."""
    h, w, mode = 96, 384, '4:2:2'
    key = (mode + '/16', False, h, w)
    img = cpu_ref.random_image(h, w, 2302)
    ref = cpu_ref.compress_reconstruct(img, Q, 16, mode, False, metrics=False, stretch=True)
    item = (cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, Q), None, 16)
    (out, cf, st, fix), = _plan(img[None], [item], mode, False, [0])
    assert np.array_equal(cf[0], ref['coeffs'])
    assert np.array_equal(out[0], ref['reconstructed'])
    _fix(key, 'full', fix)
    (out2, cf2, st2, fix2), = _plan(img[None], [item], mode, False, [0], coeffs=cf)
    assert np.array_equal(out2[0], ref['reconstructed'])
    _fix(key, 'inv', fix2)
    neg = (-cf.astype(np.int32)).astype(np.int16)
    (out4, cf4, st4, fix4), = _plan(img[None], [item], mode, False, [0], coeffs=neg)
    assert np.array_equal(out4[0], inverse_ref(neg[0], Q, mode, h, w, block=16))
    _fix(key, 'neg', fix4)
