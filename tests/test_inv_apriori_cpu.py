"""The a-priori certificate of full runs, pinned on the CPU (no GPU).

A full run's inverse reads the coefficients its own forward wrote, so
|q * Q| <= 1152 and the certified fast inverse (csrc/jds_inv_fast.hip, AP)
tests every value against a constant threshold T = ceil(E * 2^32) + 1 grid
steps of 2^-32, E = K_LIN * 1152 + K_CONST + 2^-31.  It does so one-sided: S =
T + 1 steps ride on the luma constant, every fraction word becomes lo'' = (lo +
S) mod 2^32, and a value is uncertain exactly when lo'' < 2 S.  Here:

* jds_selftest_inv_cert runs the two-sided and the one-sided form on given
  values: same verdict everywhere, same byte wherever the verdict is "certain";
* S as compiled is the one the constants give;
* the kernel's chain in offset form, on the host (jds_selftest_inv_fast, fuse
  bit 1), never certifies a byte that differs from the oracle's, on the
  adversarial frames of test_inv_bound_cpu with |q Q| <= 1152."""
import math

import numpy as np
import pytest

from oracle import cpu_ref
from test_inv_bound_cpu import MODES, _images, _planes, _reference_values

DMAX = 1152


@pytest.fixture(scope='module')
def L():
    from jds import _abi
    return _abi.lib()


def _forms(L, v):
    """(bytes[n, 2], certain[n, 2], consts[5]) of the two forms on values v."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    by = np.empty((v.size, 2), np.uint8)
    ce = np.empty((v.size, 2), np.uint8)
    consts = np.empty(5, np.float64)
    assert L.jds_selftest_inv_cert(v.ctypes.data, v.size, by.ctypes.data, ce.ctypes.data, consts.ctypes.data) == 0
    return by, ce.astype(bool), consts


@pytest.fixture(scope='module')
def consts(L):
    return _forms(L, np.zeros(1))[2]


def test_offset_as_compiled(consts):
    k_lin, k_const, dmax, T, S = consts
    assert dmax == DMAX
    want = math.ceil((k_lin * DMAX + k_const + 2.0 ** -31) * 2.0 ** 32) + 2
    assert S == want and T == S - 1, (S, T, want)
    assert 2 * S < 2 ** 16  # far below 2^32
    # the constants are the kernel's (tools/inv_bound.py reads them from the source)
    import test_inv_bound_cpu as tb
    K = tb.inv_bound.kernel_constants()
    assert K['K_LIN'] == k_lin and K['K_CONST'] == k_const


@pytest.mark.parametrize('ip', [0, 255, -1, 256, 1, 127, 254, -128, 300, 100000])
def test_one_sided_form_equals_two_sided(L, consts, ip):
    T, S = int(consts[3]), int(consts[4])
    rng = np.random.default_rng(1000 + (ip % 997))
    lo = np.concatenate([np.arange(0, 3 * S + 1), np.arange(2 ** 32 - 3 * S, 2 ** 32),
                         rng.integers(0, 2 ** 32, 100000)]).astype(np.uint64)
    v = float(ip) + lo.astype(np.float64) * 2.0 ** -32  # exact: < 52 significant bits
    assert np.array_equal(np.floor(v), np.full(v.size, float(ip)))
    by, ce, _ = _forms(L, v)
    # the two-sided form is the kernel's present test at the same T
    want_certain = ~((lo <= T) | (lo >= 2 ** 32 - 1 - T))
    assert np.array_equal(ce[:, 0], want_certain)
    assert np.array_equal(by[:, 0], np.full(v.size, np.clip(ip, 0, 255), np.uint8))
    # same verdict, and the same byte wherever it says certain
    assert np.array_equal(ce[:, 1], ce[:, 0]), np.flatnonzero(ce[:, 1] != ce[:, 0])[:5]
    assert np.array_equal(by[ce[:, 1], 1], by[ce[:, 1], 0])
    # both verdicts occur, and a carry into the integer part happens only on uncertain values
    assert ce[:, 0].any() and (~ce[:, 0]).any()
    if 0 <= ip < 255:
        assert (by[lo >= 2 ** 32 - S, 1] == ip + 1).all()


def _bounded(q, Q, mode, H, W):
    """q with every coefficient clipped to |q * Q| <= DMAX."""
    lim = np.floor(DMAX / Q).astype(np.int64).reshape(-1)
    out, off = [], 0
    for ph, pw in _planes(mode, H, W):
        n = -(-ph // 8) * -(-pw // 8) * 64
        blk = q[off:off + n].astype(np.int64).reshape(-1, 64)
        out.append(np.clip(blk, -lim, lim).reshape(-1))
        off += n
    return np.concatenate(out).astype(np.int16)


def _check_offset(L, q, Q, mode, H, W, consts, stats):
    S = int(consts[4])
    assert (np.abs(q.astype(np.int64).reshape(-1, 64)) * Q.reshape(-1) <= DMAX).all()
    v_ref, _ = _reference_values(q, Q, mode, H, W)
    ref_bytes = np.clip(v_ref, 0, 255).astype(np.uint8)
    q = np.ascontiguousarray(q, dtype=np.int16)
    Qc = np.ascontiguousarray(Q, dtype=np.float64)
    for fuse in (0, 1):
        v = np.empty((H, W, 3), np.float64)
        by = np.empty((H, W, 3), np.uint8)
        assert L.jds_selftest_inv_fast(MODES[mode], q.ctypes.data, Qc.ctypes.data, H, W, fuse | 2, v.ctypes.data,
                                       by.ctypes.data) == 0
        # values carry the offset: on the 2^-32 grid, within E + S 2^-32 of the reference
        lo = (v - np.floor(v)) * 2.0 ** 32
        assert np.array_equal(lo, np.rint(lo))
        assert np.array_equal(by, np.clip(np.floor(v), 0, 255).astype(np.uint8))
        cert = lo >= 2 * S
        stats['values'] += cert.size
        stats['certified'] += int(cert.sum())
        bad = cert & (by != ref_bytes)
        assert not bad.any(), (mode, fuse, np.argwhere(bad)[:5])
        # and the plain form's bytes are the same wherever the offset form is certain
        v0 = np.empty((H, W, 3), np.float64)
        b0 = np.empty((H, W, 3), np.uint8)
        assert L.jds_selftest_inv_fast(MODES[mode], q.ctypes.data, Qc.ctypes.data, H, W, fuse, v0.ctypes.data,
                                       b0.ctypes.data) == 0
        assert np.array_equal(by[cert], b0[cert])
        # (<= 3 roundings on the grid, each may resolve a tie the other way: one step each)
        assert np.abs(v - S * 2.0 ** -32 - v0).max() <= 3 * 2.0 ** -32


@pytest.mark.parametrize('mode', list(MODES))
def test_offset_chain_certifies_only_oracle_bytes(L, consts, mode):
    H, W = 40, 72
    stats = {'values': 0, 'certified': 0}
    for name, img in _images(H, W).items():
        for quality in (1, 10, 50, 95, 100):
            for pf in ((False, True) if mode != '4:4:4' else (False,)):
                out = cpu_ref.compress_reconstruct(img, quality, 8, mode, pf, metrics=False)
                Q = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, quality)
                # codec output: within the bound as it stands
                _check_offset(L, np.asarray(out['coeffs'], np.int16), Q, mode, H, W, consts, stats)
    # arbitrary coefficients scaled into the bound: every |q Q| as large as it may be
    rng = np.random.default_rng(17)
    n = sum(-(-ph // 8) * -(-pw // 8) * 64 for ph, pw in _planes(mode, H, W))
    cases = [rng.integers(-32768, 32768, n), rng.choice([-32767, 32767], n),
             np.where(rng.random(n) < 0.05, rng.choice([-32767, 32767], n), rng.integers(-2, 3, n))]
    for q in cases:
        for quality in (1, 50, 100):
            Q = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, quality)
            _check_offset(L, _bounded(q, Q, mode, H, W), Q, mode, H, W, consts, stats)
    print(f"{mode}: {stats['certified']} / {stats['values']} values certified in offset form")
    assert stats['certified'] > 0.5 * stats['values']
