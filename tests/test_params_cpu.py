"""Tables and taps other than the defaults, on the CPU (no GPU).

Every other codec test runs scale_quant_matrix(JPEG_LUMA_Q50, q) and
gaussian_kernel3(0.75).  The C ABI takes any integer table in [1, 255] and any
symmetric finite taps, and the values feed the certificates: the fp32
forward's bounds (fast_fwd_bounds / fast_fwd16_bounds, from the taps), its
certification limits (from Q), the certified inverse's tracked and fixed
bounds.  Here, with params_ref (the oracle's stage functions with the table and
the taps as arguments) as the reference:

* params_ref with the defaults is cpu_ref.compress_reconstruct;
* the forward's host chain stays within its bound for every accepted taps
  vector, signed ones and ones whose sum is not 1 included, and certifies only
  the reference's roundings at every table of params_cases.TABLES;
* the bounds of the default taps are the recorded ones, bit for bit
  (tests/golden/fwd_bounds_default.npz);
* the certified inverse's host chain stays within its bound on the
  coefficients of every table, in the tracked and in the a-priori form;
* max |q Q| <= 1152 wherever the plan assumes it, and not for a sharpening
  prefilter, where the plan must not;
* asymmetric and non-finite taps are refused by name whenever the prefilter
  runs (jds_geometry_of; host only)."""
import os
import re

import numpy as np
import pytest

import params_ref
from oracle import cpu_ref
from params_cases import BAD_TAPS, TABLES, TAPS, _bound_inputs, apriori_ok
from test_cert_bound_cpu import BLOCKS, IMAGES, _thr
from test_inv_apriori_cpu import DMAX, _check_offset
from test_inv_bound_cpu import _check, _images, inv_bound

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fwd_bounds_default.npz')
CODES = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
DEFAULT_Q = {q: cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q) for q in (10, 50, 95)}
DEFAULT_TAPS = cpu_ref.gaussian_kernel3(0.75)


@pytest.fixture(scope='module')
def L():
    from jds import _abi
    return _abi.lib()


# ---- the helper is the oracle ---------------------------------------------------

def _same_as_oracle(img, q, bs, mode, pf):
    ref = cpu_ref.compress_reconstruct(img, q, bs, mode, pf, metrics=False, stretch=bs == 16)
    got = params_ref.compress_reconstruct(img, DEFAULT_Q[q], mode, pf, DEFAULT_TAPS, bs)
    assert got['coeffs'].dtype == ref['coeffs'].dtype and np.array_equal(got['coeffs'], ref['coeffs'])
    assert np.array_equal(got['reconstructed'], ref['reconstructed'])
    assert np.array_equal(got['hist'], ref['hist'])
    assert got['bitrate'] == ref['bitrate']  # nonzero_count and every other field
    assert np.array_equal(got['error_map_y'], ref['error_map_y'])


@pytest.mark.parametrize('h,w', [(40, 72), (37, 53)])
@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2', '4:4:4'])
def test_params_ref_with_defaults_is_the_oracle(h, w, mode):
    img = cpu_ref.random_image(h, w, 2200 + h)
    for pf in (False, True):
        for q in (10, 50, 95):
            _same_as_oracle(img, q, 8, mode, pf)


def test_params_ref_with_defaults_is_the_oracle_16x16():
    _same_as_oracle(cpu_ref.random_image(40, 72, 2201), 50, 16, '4:2:0', True)


# ---- the forward certificate ----------------------------------------------------

def fwd_chain(L, bs, code, pf, taps, img, plane, flags):
    """(c32[n, bs * bs], bound[bs * bs]) of jds_selftest_fwd32 / fwd16."""
    sy, sx = (2 if code == 2 else 1), (1 if code == 0 else 2)
    ph, pw = (img.shape[0], img.shape[1]) if plane == 0 else (img.shape[0] // sy, img.shape[1] // sx)
    c32 = np.empty(((ph // bs) * (pw // bs), bs * bs), np.float32)
    bound = np.empty(bs * bs, np.float64)
    taps = np.ascontiguousarray(taps, np.float64)
    rc = getattr(L, BLOCKS[bs])(code, int(pf), taps.ctypes.data, img.ctypes.data, img.shape[0], img.shape[1], plane,
                                flags, c32.ctypes.data, bound.ctypes.data)
    assert rc == 0
    return c32, bound


def fwd_bounds(L, bs, code, pf, plane, taps):
    return fwd_chain(L, bs, code, pf, taps, np.zeros((32, 32, 3), np.uint8), plane, 3)[1]


@pytest.mark.parametrize('bs', [8, 16])
@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2'])
@pytest.mark.parametrize('taps', sorted(TAPS))
def test_fp32_forward_error_within_certified_bound_per_taps(L, taps, mode, bs):
    """test_cert_bound_cpu's check with the prefilter's taps and the table as
    parameters: |c_fp32 - c_exact| < E, and no certified rounding differs from
    np.round(c_exact / Q), at every table."""
    gk = TAPS[taps]
    worst = 0.0
    accepted = accepted_chroma = wrong = 0
    tables = {n: (np.kron(Q, np.ones((2, 2))) if bs == 16 else Q).reshape(-1) for n, Q in TABLES.items()}
    for name, img in IMAGES.items():
        img = np.ascontiguousarray(img)
        planes = params_ref.planes(img, mode, True, gk)
        for plane in range(3):
            exact = cpu_ref.encode_blocks(cpu_ref.split_blocks(planes[plane], bs)).reshape(-1, bs * bs)
            for flags in (3, 2):  # the combined-tap chain, rows or columns first
                c32, bound = fwd_chain(L, bs, CODES[mode], True, gk, img, plane, flags)
                ratio = np.abs(c32.astype(np.float64) - exact) / bound
                worst = max(worst, float(ratio.max()))
                assert ratio.max() < 1.0, (name, plane, flags, float(ratio.max()))
                for Q in tables.values():
                    t = c32 * (1.0 / Q).astype(np.float32)
                    r = np.rint(t)
                    ok = np.abs(t - r) < (_thr(bound, Q) - np.abs(t) * np.float32(2.0 ** -22))
                    accepted += int(ok.sum())
                    accepted_chroma += int(ok.sum()) if plane else 0
                    wrong += int(np.sum(ok & (r != np.round(exact / Q))))
    print(f'{taps} {bs}x{bs} {mode}: worst |c32 - c_exact| / E = {worst:.4f}; {accepted} certified roundings '
          f'({accepted_chroma} chroma), {wrong} wrong; max chroma E = {bound.max():.4g}')
    assert wrong == 0
    assert accepted > 0
    if taps in ('sub1', 'over1'):
        # the level shift's 128 |S^2 - 1| alone exceeds Q / 2 at Q = 255: every
        # chroma block goes to the exact fix-up (test_gpu_params counts them)
        assert accepted_chroma == 0
    else:
        assert accepted_chroma > 0


def test_default_bounds_are_the_recorded_ones(L):
    """No threshold of the default configuration moves: the bound arrays of
    gaussian_kernel3(0.75), recorded before fwd_input_error took signed taps."""
    g = np.load(GOLDEN)
    n = 0
    for bs in (8, 16):
        for code in (0, 1, 2):
            for pf in (0, 1):
                for plane in (0, 1):
                    want = g[f'b{bs}_m{code}_pf{pf}_p{plane}']
                    got = fwd_bounds(L, bs, code, pf, plane, DEFAULT_TAPS)
                    assert want.shape == (bs * bs,) and want.dtype == np.float64
                    assert got.tobytes() == want.tobytes(), (bs, code, pf, plane)
                    n += 1
    assert n == len(g.files) == 24


# ---- the certified inverse on the coefficients of every table -------------------

@pytest.fixture(scope='module')
def model():
    res, k_lin, k_const = inv_bound.bounds()
    return k_lin, k_const


@pytest.fixture(scope='module')
def consts(L):
    c = np.empty(5, np.float64)
    v, by, ce = np.zeros(1), np.empty((1, 2), np.uint8), np.empty((1, 2), np.uint8)
    assert L.jds_selftest_inv_cert(v.ctypes.data, 1, by.ctypes.data, ce.ctypes.data, c.ctypes.data) == 0
    return c


INV_H, INV_W = 40, 72
INV_IMAGES = _images(INV_H, INV_W)
INV_TAPS = [None] + [t for t in sorted(TAPS) if apriori_ok(TAPS[t])]  # None: no prefilter


@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2', '4:4:4'])
@pytest.mark.parametrize('table', sorted(TABLES))
def test_inverse_chain_within_bound_per_table(L, model, consts, table, mode):
    """test_inv_bound_cpu's _check (tracked bound, both fuse forms) and
    test_inv_apriori_cpu's _check_offset (fuse bit 1: the fixed bound of full
    runs) on what the forward writes at this table."""
    Q = TABLES[table]
    stats = {'worst': 0.0, 'worst_model': 0.0, 'values': 0, 'certified': 0}
    ostats = {'values': 0, 'certified': 0}
    for name, img in INV_IMAGES.items():
        for t in (INV_TAPS if mode != '4:4:4' else [None]):
            # the default taps on every image; the others where a prefilter acts: colour edges
            if t not in (None, 'gauss075') and name not in ('extremes', 'checker1', 'red_blue_edge'):
                continue
            taps = DEFAULT_TAPS if t is None else TAPS[t]
            out = params_ref.compress_reconstruct(img, Q, mode, t is not None, taps)
            ref_bytes = _check(L, out['coeffs'], Q, mode, INV_H, INV_W, model, stats)
            assert np.array_equal(ref_bytes, out['reconstructed']), (name, t)
            _check_offset(L, np.asarray(out['coeffs'], np.int16), Q, mode, INV_H, INV_W, consts, ostats)
    # sharpening taps: coefficients beyond the fixed bound, the tracked form alone
    for t in ('sharp', 'sharp2'):
        if mode != '4:4:4':
            out = params_ref.compress_reconstruct(INV_IMAGES['extremes'], Q, mode, True, TAPS[t])
            ref_bytes = _check(L, out['coeffs'], Q, mode, INV_H, INV_W, model, stats)
            assert np.array_equal(ref_bytes, out['reconstructed']), t
    print(f"{table} {mode}: worst |v_fast - v_ref| / E = {stats['worst']:.3e}; {stats['certified']} / "
          f"{stats['values']} values certified (tracked), {ostats['certified']} / {ostats['values']} (a-priori)")


# ---- the a-priori premise ---------------------------------------------------------

def _max_qQ(frames, mode, pf, taps):
    """{table: max |q Q|} over the params_ref coefficients of the frames."""
    worst = dict.fromkeys(TABLES, 0.0)
    for img in frames:
        dct, _ = params_ref.dct_planes(img, mode, pf, taps)
        for name, Q in TABLES.items():
            for c, _, _ in dct:
                worst[name] = max(worst[name], float(np.abs(cpu_ref.dequantize(cpu_ref.quantize(c, Q), Q)).max()))
    return worst


@pytest.fixture(scope='module')
def bound_frames():
    return _bound_inputs(64, 128)


@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2', '4:4:4'])
def test_forward_output_within_the_fixed_bound_where_the_plan_assumes_it(bound_frames, mode):
    """|c| <= 8 * 128 and |q Q| <= |c| + Q / 2 <= 1152 for every table without a
    prefilter and with non-negative taps of sum <= 1 (jds_plan's apriori_ok)."""
    cases = [(False, DEFAULT_TAPS)]
    if mode != '4:4:4':
        cases += [(True, TAPS[t]) for t in sorted(TAPS) if apriori_ok(TAPS[t])]
    top = 0.0
    for pf, taps in cases:
        for name, v in _max_qQ(bound_frames, mode, pf, taps).items():
            assert v <= DMAX, (name, pf, list(taps), v)
            top = max(top, v)
    print(f'{mode}: max |q Q| = {top:g} over {len(cases)} prefilter settings x {len(TABLES)} tables')
    assert top >= 1000  # the inputs do reach the codec's magnitudes


@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2'])
def test_sharpening_taps_leave_the_fixed_bound(bound_frames, mode):
    """sharp2 at flat1: the regime the fixed bound excludes (the plan's
    apriori_ok is false; test_gpu_params runs it on the device)."""
    assert not apriori_ok(TAPS['sharp2']) and not apriori_ok(TAPS['sharp']) and not apriori_ok(TAPS['over1'])
    v = _max_qQ(bound_frames, mode, True, TAPS['sharp2'])['flat1']
    print(f'{mode}: sharp2 at flat1: max |q Q| = {v:g}')
    assert v > DMAX


# ---- refusals (host only) ---------------------------------------------------------

def _geo(taps, mode, pf, bs=8, h=64, w=128):
    from jds import _abi
    g = _abi.geometry(_abi.make_params(50, DEFAULT_Q[50], mode, pf, np.asarray(taps, np.float64), bs), h, w)
    return [getattr(g, f[0]) for f in g._fields_]


@pytest.mark.parametrize('bad', sorted(BAD_TAPS))
def test_bad_taps_refused_when_the_prefilter_runs(bad):
    taps = BAD_TAPS[bad]
    for mode in ('4:2:0', '4:2:2'):
        for bs in (8, 16):
            with pytest.raises(ValueError, match=r'prefilter taps \[.*\] must be finite and symmetric') as e:
                _geo(taps, mode, True, bs)
            # the message prints the taps
            shown = [float(x) for x in re.search(r'\[(.*?)\]', str(e.value)).group(1).split(',')]
            assert np.array_equal(shown, taps, equal_nan=True), str(e.value)
        # ignored without the prefilter ...
        assert _geo(taps, mode, False) == _geo(DEFAULT_TAPS, mode, False)
    # ... and at 4:4:4, whatever the flag says
    assert _geo(taps, '4:4:4', True) == _geo(DEFAULT_TAPS, '4:4:4', True) == _geo(DEFAULT_TAPS, '4:4:4', False)


@pytest.mark.parametrize('taps', sorted(TAPS))
def test_symmetric_taps_accepted(taps):
    for mode in ('4:2:0', '4:2:2'):
        assert _geo(TAPS[taps], mode, True) == _geo(DEFAULT_TAPS, mode, True)
