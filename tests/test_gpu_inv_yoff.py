"""4:2:0 inverse tiles raised by one luma block row, and the level-shifted
forward chroma chains, against the oracle (all 4:2:0 unless named).

The tiled inverses (k_inv_fast, its exact tile body inv2_tile, k_inv2) start
their 64 x 128 tiles 8 luma rows above 64 ty where that adds no tile row
(csrc/jds_internal.hpp inv_tile_yoff): the chroma window then takes five block
rows instead of six.  Heights 56, 120 and 184 take the offset with one, two and
three tile rows; 64 and 128 must fall back to aligned tiles; width 144 has a
partial last tile column.  Every inverse route must give the oracle's bytes:
the plan's own (certified fast), the exact kernel, and the fast kernel with
every tile recomputed by the exact tile body (RUN_INV_FIXALL), which drives the
fallback through the raised geometry.  Flat and saturated frames send every tile
to that fallback by themselves.

The forward kernels form Cb - 128 / Cr - 128 directly (csrc/jds_fwd_common.hpp
cb32m / cr32m) and certify with a tighter chroma bound: coefficients and
statistics must still equal the oracle's on random frames, on exact ties (flat
odd gray) and on saturated colours, and equal the all-fp64 RUN_EXACT kernels'."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu

HEIGHTS = {56: (8, 1), 120: (8, 2), 184: (8, 3), 64: (0, 1), 128: (0, 2)}  # H: (offset, tile rows)
WIDTHS = (128, 144)
Q = 50


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


@functools.lru_cache(maxsize=None)
def _frames(h, w):
    return np.stack([cpu_ref.random_image(h, w, 4200 + h + w + i) for i in range(2)])


@functools.lru_cache(maxsize=None)
def _refs(h, w, mode='4:2:0'):
    return [cpu_ref.compress_reconstruct(f, Q, 8, mode, True, metrics=False) for f in _frames(h, w)]


def _run(frames, mode, flag_seq, qs=None, nq=1):
    """One plan; the runs of flag_seq in order on the same buffers (a RUN_INV run
    reads the coefficients the run before it left).  Returns [(out, cf, stats, fix)]."""
    import torch
    from jds import _abi, codec
    n, H, W = frames.shape[:3]
    qs = qs or [Q]
    params = [_abi.make_params(q, cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q), mode, True,
                               codec.gaussian_kernel3()) for _ in range(n) for q in qs]
    plan = _abi.Plan(_abi.context(0), params, H, W, nq=nq) if nq > 1 else _abi.Plan(_abi.context(0), params, H, W)
    dev = torch.device('cuda:0')
    rgb = torch.from_numpy(np.ascontiguousarray(frames if nq > 1 else np.repeat(frames, len(qs), axis=0))).to(dev)
    out = torch.zeros((len(params), H, W, 3), dtype=torch.uint8, device=dev)
    cf = torch.zeros((len(params), plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
    st = torch.zeros((len(params), _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    res = []
    for flags in flag_seq:
        if flags & _abi.RUN_INV:
            out.zero_()
        plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), flags,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), cf.cpu().numpy(), st.cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1).copy(),
                    plan.fix_counts()))
    plan.close()
    return res


def _tiles(h, w):
    return ((h + 63) // 64) * ((w + 127) // 128)


@pytest.mark.parametrize('h', sorted(HEIGHTS))
def test_heights_take_the_expected_offset(h):
    from jds import _abi
    out = (C.c_int32 * 8)()
    assert _abi.lib().jds_selftest_inv_rows(2, h, 0, out, None) == 0
    assert (out[0], out[1]) == HEIGHTS[h]


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('h', sorted(HEIGHTS))
def test_plan_run_equals_oracle(h, w):
    (out, cf, st, fix), = _run(_frames(h, w), '4:2:0', [0])
    for i, ref in enumerate(_refs(h, w)):
        assert np.array_equal(cf[i], ref['coeffs']), i
        assert np.array_equal(out[i], ref['reconstructed']), (i, int(np.sum(out[i] != ref['reconstructed'])))


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('h', sorted(HEIGHTS))
def test_inverse_routes_equal_oracle(h, w):
    from jds import _abi
    A = _abi
    res = _run(_frames(h, w), '4:2:0', [A.RUN_FWD, A.RUN_INV, A.RUN_INV | A.RUN_EXACT_INV,
                                        A.RUN_INV | A.RUN_INV_FIXALL])
    refs = _refs(h, w)
    for i, ref in enumerate(refs):
        assert np.array_equal(res[0][1][i], ref['coeffs']), i
    for name, (out, cf, st, fix) in zip(('fast', 'exact', 'fixall'), res[1:]):
        for i, ref in enumerate(refs):
            assert np.array_equal(out[i], ref['reconstructed']), (name, i, int(np.sum(out[i] != ref['reconstructed'])))
    assert res[3][3][1] == 2 * _tiles(h, w)  # every tile went through the exact tile body


@pytest.mark.parametrize('kind', ['gray', 'saturated'])
def test_fallback_in_raised_tiles(kind):
    """Flat gray and saturated frames reconstruct to exact integers: every tile
    of the certified kernel is uncertain and recomputed by the exact tile body."""
    h, w = 120, 144
    img = np.full((h, w, 3), 128, np.uint8) if kind == 'gray' else np.full((h, w, 3), 255, np.uint8)
    if kind == 'saturated':  # white over black with a red stripe: every tile holds white or black blocks
        img[h // 2:] = 0
        img[:, 40:60] = (255, 0, 0)
    frames = np.stack([img, img])
    (out, cf, st, fix), = _run(frames, '4:2:0', [0])
    ref = cpu_ref.compress_reconstruct(img, Q, 8, '4:2:0', True, metrics=False)
    for i in range(2):
        assert np.array_equal(cf[i], ref['coeffs'])
        assert np.array_equal(out[i], ref['reconstructed']), int(np.sum(out[i] != ref['reconstructed']))
    assert fix[1] == 2 * _tiles(h, w), fix


def test_sweep_sse_equals_exact_kernels():
    from jds import _abi
    h, w = 120, 144
    qs = [20, 50, 90]
    frames = _frames(h, w)
    (o_s, c_s, s_s, _), = _run(frames, '4:2:0', [_abi.RUN_SSE], qs=qs, nq=len(qs))
    (o_x, c_x, s_x, _), = _run(frames, '4:2:0', [_abi.RUN_SSE | _abi.RUN_EXACT], qs=qs, nq=len(qs))
    assert np.array_equal(o_s, o_x) and np.array_equal(c_s, c_x)
    assert np.array_equal(s_s['sse_rgb'], s_x['sse_rgb'])
    assert np.array_equal(s_s['sse_y'].view(np.uint64), s_x['sse_y'].view(np.uint64))
    want = [int(((frames[i // len(qs)].astype(np.int64) - o_x[i]) ** 2).sum()) for i in range(len(o_x))]
    assert [int(v) for v in s_s['sse_rgb']] == want


def _fwd_image(kind, h, w):
    if kind == 'random':
        return cpu_ref.random_image(h, w, 77 + h)
    if kind == 'gray127':
        return np.full((h, w, 3), 127, np.uint8)
    cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                     [255, 255, 255], [0, 0, 0]], np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return cols[((yy // 5) * 3 + xx // 7) % len(cols)]


@pytest.mark.parametrize('kind', ['random', 'gray127', 'colours'])
@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2'])
@pytest.mark.parametrize('h,w', [(64, 128), (120, 144)])
def test_forward_equals_oracle(h, w, mode, kind):
    from jds import _abi
    img = _fwd_image(kind, h, w)
    frames = np.stack([img, img[::-1].copy()])
    fast, exact = _run(frames, mode, [_abi.RUN_FWD, _abi.RUN_FWD | _abi.RUN_EXACT])
    for i in range(2):
        ref = cpu_ref.compress_reconstruct(frames[i], Q, 8, mode, True, metrics=False)
        for name, (out, cf, st, fix) in (('fast', fast), ('exact', exact)):
            assert np.array_equal(cf[i], ref['coeffs']), (name, i, int(np.sum(cf[i] != ref['coeffs'])))
            assert st[i]['nonzero'] == ref['bitrate']['nonzero_count'], (name, i)
            assert np.array_equal(st[i]['hist'], ref['hist']), (name, i)
    for fld in ('nonzero', 'magnitude_bits', 'hist'):
        assert np.array_equal(fast[2][fld], exact[2][fld]), fld
