"""The certified forward's chroma bound after the chains moved to level-shifted
samples (CPU, no GPU).

cb32m / cr32m (csrc/jds_fwd_common.hpp) form Cb - 128 and Cr - 128 directly, the
prefilter and area chains run on |x| <= 128 and end without a subtraction, and
fwd_input_error prices every rounding at half the former magnitude plus
128 |S^2 - 1| for the Gaussian taps' sum.  Checked through the host restatement
of the kernels' chain (jds_selftest_fwd32) on test_cert_bound_cpu's adversarial
images: |c_fp32 - c_exact| <= E_uv for every coefficient, both pass orders,
4:2:0 and 4:2:2, prefilter on and off.  The second test counts, on the host,
the chroma blocks of a seeded random 1080p frame that the certificate lists at
Q50 with the bound as it was (tests/golden/fwd_chroma_bound_before.json, recorded
from the previous fast_fwd_bounds) and as it is."""
import json
import os

import numpy as np
import pytest

from oracle import cpu_ref
from test_cert_bound_cpu import IMAGES, _exact_planes, _thr

BEFORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fwd_chroma_bound_before.json')


@pytest.fixture(scope='module')
def L():
    from jds import _abi
    return _abi.lib()


def _fwd32(L, code, pf, img, plane, flags):
    gk = cpu_ref.gaussian_kernel3(0.75)
    sy, sx = (2 if code == 2 else 1), (1 if code == 0 else 2)
    ph, pw = (img.shape[0], img.shape[1]) if plane == 0 else (img.shape[0] // sy, img.shape[1] // sx)
    c32 = np.empty(((ph // 8) * (pw // 8), 64), np.float32)
    bound = np.empty(64, np.float64)
    img = np.ascontiguousarray(img)
    rc = L.jds_selftest_fwd32(code, int(pf), gk.ctypes.data, img.ctypes.data, img.shape[0], img.shape[1], plane, flags,
                              c32.ctypes.data, bound.ctypes.data)
    assert rc == 0
    return c32, bound


@pytest.mark.parametrize('mode,pf', [('4:2:0', True), ('4:2:0', False), ('4:2:2', True), ('4:2:2', False)])
def test_chroma_error_within_bound(L, mode, pf):
    code = {'4:2:2': 1, '4:2:0': 2}[mode]
    worst = 0.0
    for name, img in IMAGES.items():
        planes = _exact_planes(np.ascontiguousarray(img), mode, pf)
        for plane in (1, 2):
            exact = cpu_ref.encode_blocks(cpu_ref.split_blocks(planes[plane], 8)).reshape(-1, 64)
            for flags in (3, 2):  # rows first / columns first, the combined taps the kernels compute
                c32, bound = _fwd32(L, code, pf, img, plane, flags)
                err = np.abs(c32.astype(np.float64) - exact)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (name, plane, flags, float((err / bound).max()))
    print(f'{mode} pf={pf}: worst chroma |c32 - c_exact| / E = {worst:.4f}')


def test_chroma_bound_is_tighter_than_before(L):
    before = json.load(open(BEFORE))['bounds']
    img = np.zeros((16, 16, 3), np.uint8)
    for mode, code in (('4:2:0', 2), ('4:2:2', 1)):
        for pf in (1, 0):
            _, now = _fwd32(L, code, pf, img, 1, 3)
            was = np.array(before[f'{mode}|pf={pf}'])
            print(f'{mode} pf={pf}: chroma E_uv max {was.max():.4e} -> {now.max():.4e}')
            assert np.all(now < was)


def _listed(c32, bound, Q):
    """Blocks with a coefficient the certificate does not accept (the kernels' test,
    as test_cert_bound_cpu restates it)."""
    t = c32 * (1.0 / Q).astype(np.float32)
    ok = np.abs(t - np.rint(t)) < (_thr(bound, Q) - np.abs(t) * np.float32(2.0 ** -22))
    return int(np.sum(~ok.all(axis=1)))


def test_fewer_chroma_blocks_listed_on_random_1080p(L):
    """The rows of a seeded random 1080p frame whose chroma planes are whole
    blocks (1072 of 1080), Q50, 4:2:0, prefilter on."""
    img = cpu_ref.random_image(1080, 1920, 2024)[:1072]
    Q = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50).reshape(-1).astype(np.float64)
    was = np.array(json.load(open(BEFORE))['bounds']['4:2:0|pf=1'])
    old = new = blocks = 0
    for plane in (1, 2):
        c32, bound = _fwd32(L, 2, True, img, plane, 3)
        blocks += len(c32)
        old += _listed(c32, was, Q)
        new += _listed(c32, bound, Q)
    print(f'chroma blocks listed of {blocks}: {old} with the former bound, {new} now')
    assert 0 < new < old
