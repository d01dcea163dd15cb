"""The a-priori certificate of full runs (csrc/jds_inv_fast.hip, AP).

A plan run of both phases in one call hands the certified fast inverse the
coefficients its own forward wrote, so |q * Q| <= 1152 and the 8x8 kernels
test every value against a constant threshold, one-sided (InvFix::apriori; the
arithmetic is pinned on the CPU in test_inv_apriori_cpu.py).  Here, on the
device: full runs equal the exact kernels and the oracle; the forward's output
stays within the bound on the inputs that reach it; exact ties are still handed
to the exact tile code; inverse-only runs on arbitrary coefficients keep the
tracked bound; the two phases as two calls, and JDS_RUN_INV_FIXALL, give the
full run's bytes."""
import numpy as np
import pytest

from oracle import cpu_ref
from params_cases import _bound_inputs  # (shared with test_params_cpu.py, which imports no GPU module)
from test_gpu_inv_fast import _plan, _same

pytestmark = pytest.mark.gpu

DMAX = 1152
STAT_FIELDS = ('nonzero', 'magnitude_bits', 'hist', 'total_coeffs')


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def _table(q):
    return cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)


# 4:2:0: one aligned tile; raised tiles (ceil((H + 8) / 64) == ceil(H / 64)); ragged on both axes
SHAPES = [(64, 128, '4:2:0'), (120, 256, '4:2:0'), (72, 136, '4:2:0'), (32, 136, '4:2:2'), (24, 40, '4:4:4')]


@pytest.mark.parametrize('q', [14, 50, 90, 100])
@pytest.mark.parametrize('h,w,mode', SHAPES)
def test_full_run_equals_exact_and_oracle(h, w, mode, q):
    from jds import _abi
    pf = mode != '4:4:4'
    frames = np.stack([cpu_ref.random_image(h, w, 1300 + i) for i in range(2)])
    full, exact = _plan(frames, [q, q], mode, pf, [0, _abi.RUN_EXACT])
    _same(full, exact)
    for f in STAT_FIELDS:
        assert np.array_equal(full[2][f], exact[2][f]), f
    for i in range(2):
        ref = cpu_ref.compress_reconstruct(frames[i], q, 8, mode, pf, metrics=False)
        assert np.array_equal(full[1][i], ref['coeffs']), i
        assert np.array_equal(full[0][i], ref['reconstructed']), i
        assert [int(v) for v in full[2][i]['hist']] == [int(v) for v in ref['hist']]
        assert int(full[2][i]['nonzero']) == ref['bitrate']['nonzero_count']


@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2', '4:4:4'])
def test_forward_output_within_the_bound(mode):
    """max |q * Q| over the forward's coefficients, on the host: the premise
    of the fixed bound (|c| <= 8 * 128, |q Q| <= |c| + Q / 2)."""
    from jds import _abi
    h, w = 64, 128
    inputs = _bound_inputs(h, w)
    pf = mode != '4:4:4'
    worst = 0
    for q in (100, 50, 14):
        full, exact = _plan(inputs, [q] * len(inputs), mode, pf, [0, _abi.RUN_EXACT_INV])
        Q = _table(q).reshape(-1).astype(np.int64)
        qq = np.abs(full[1].astype(np.int64).reshape(len(inputs), -1, 64)) * Q
        worst = max(worst, int(qq.max()))
        assert qq.max() <= DMAX, (q, int(qq.max()), int(np.argmax(qq.max(axis=(1, 2)))))
        _same(full, exact)
    print(f'{mode}: max |q Q| = {worst}')
    assert worst >= 1000  # the inputs do reach the codec's magnitudes


def _tie_frames(h, w):
    gray = np.full((h, w, 3), 128, np.uint8)
    sat = np.zeros((h, w, 3), np.uint8)
    sat[:, w // 2:] = 255
    rng = np.random.default_rng(1500)
    lv = rng.integers(0, 256, (-(-h // 16), -(-w // 16)), dtype=np.uint8)
    mcu = np.kron(lv, np.ones((16, 16), np.uint8))[:h, :w]
    return {'gray128': gray, 'saturated': sat, 'mcu_constant': np.stack([mcu, mcu, mcu], axis=-1)}


@pytest.mark.parametrize('name', ['gray128', 'saturated', 'mcu_constant'])
@pytest.mark.parametrize('mode', ['4:2:0', '4:4:4'])
def test_ties_take_the_fallback(mode, name):
    """Reference values that are integers up to pocketfft noise: the full run
    must hand those tiles to the exact tile code (without this the equality
    above could pass while the fallback is never taken)."""
    from jds import _abi
    img = _tie_frames(64, 128)[name]
    frames = np.stack([img, img])
    full, exact = _plan(frames, [50, 50], mode, mode != '4:4:4', [0, _abi.RUN_EXACT])
    assert full[3][1] > 0, full[3]
    _same(full, exact)
    ref = cpu_ref.compress_reconstruct(img, 50, 8, mode, mode != '4:4:4', metrics=False)
    assert np.array_equal(full[0][0], ref['reconstructed'])


@pytest.mark.parametrize('mode', ['4:2:0', '4:4:4'])
def test_inverse_only_keeps_the_tracked_bound(mode):
    """Inverse-only runs on arbitrary int16 coefficients (|q Q| far above 1152)
    equal the exact inverse: the fixed bound is a full run's alone."""
    from jds import _abi, codec
    h, w = 64, 128
    frames = np.stack([cpu_ref.random_image(h, w, 1600 + i) for i in range(2)])
    cpf = _abi.geometry(_abi.make_params(50, _table(50), mode, mode != '4:4:4', codec.gaussian_kernel3()),
                        h, w).coeffs_per_frame
    rng = np.random.default_rng(1601)
    for cf in (rng.integers(-32768, 32768, (2, cpf)).astype(np.int16),
               np.clip(rng.normal(0, 400, (2, cpf)), -32768, 32767).astype(np.int16)):
        assert (np.abs(cf.astype(np.int64)).max() * 16) > 10 * DMAX
        fast, exact = _plan(frames, [50, 90], mode, mode != '4:4:4', [0, _abi.RUN_EXACT_INV], coeffs=cf)
        _same(fast, exact)


def _two_calls(frames, qs, mode, pf):
    """JDS_RUN_FWD then JDS_RUN_INV as two calls on one plan."""
    import torch
    from jds import _abi, codec
    H, W = frames.shape[1:3]
    params = [_abi.make_params(q, _table(q), mode, pf, codec.gaussian_kernel3()) for q in qs]
    plan = _abi.Plan(_abi.context(0), params, H, W)
    dev = torch.device('cuda:0')
    rgb = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    out = torch.zeros_like(rgb)
    cf = torch.empty((len(qs), plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
    st = torch.zeros((len(qs), _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), _abi.RUN_FWD, 0)
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), _abi.RUN_INV, 0)
    torch.cuda.synchronize()
    res = (out.cpu().numpy(), cf.cpu().numpy(), st.cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1),
           plan.fix_counts())
    plan.close()
    return res


@pytest.mark.parametrize('h,w,mode', [(72, 136, '4:2:0'), (32, 136, '4:2:2'), (24, 40, '4:4:4')])
def test_phases_as_two_calls_and_fixall_equal_the_full_run(h, w, mode):
    from jds import _abi
    pf = mode != '4:4:4'
    frames = np.stack([cpu_ref.random_image(h, w, 1700), _tie_frames(h, w)['saturated']])
    full, fixall = _plan(frames, [50, 90], mode, pf, [0, _abi.RUN_INV_FIXALL])
    split = _two_calls(frames, [50, 90], mode, pf)
    _same(split, full)
    _same(fixall, full)
    for f in STAT_FIELDS:
        assert np.array_equal(split[2][f], full[2][f]) and np.array_equal(fixall[2][f], full[2][f]), f
    assert fixall[3][1] >= full[3][1] and fixall[3][1] > 0  # every tile (4:4:4: wave) was recomputed
