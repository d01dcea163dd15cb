"""CPU checks of the fused inverse for foreign JPEGs (no GPU): the kernel's tile core
(csrc/jds_jpeg_inv.hpp) run by a host tile loop (jds_selftest_jpeg_inverse) against the
definition of the staged inverse (test_jpeg_interleaved_cpu.oracle_image), the chroma window
function against NumPy's taps, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import interleaved_ref as ir
from oracle import cpu_ref
from test_jpeg_interleaved_cpu import NAMES, Q50, QC, fixture, oracle_image

Q2 = np.clip(QC + 7, 1, 255)
QT = np.stack([Q50, QC, Q2])           # three distinct tables, tq = (0, 1, 2)
MODES = ['4:2:0', '4:2:2', '4:4:4']
SETTINGS = {'saturating': dict(amp=300, density=0.9), 'interior': dict(amp=40, density=0.3)}
SMALL = list(range(1, 19)) + [31, 32, 33]


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def tile():
    from jds import codec
    return codec.jpeg_inverse_info()


def planar(rng, H, W, mode, **kw):
    grids = ir.geometry(H, W, mode)[1]
    return ir.crop(ir.random_padded(rng, H, W, mode, **kw), grids), grids


def both(rng, H, W, mode, **kw):
    from jds import codec
    cf, grids = planar(rng, H, W, mode, **kw)
    return codec.host_jpeg_inverse(cf, H, W, mode, QT, grids), oracle_image(cf, H, W, mode, QT, grids)


def test_tile_is_a_multiple_of_16():
    th, tw = tile()
    assert th > 0 and tw > 0 and th % 16 == 0 and tw % 16 == 0


@pytest.mark.parametrize('setting', sorted(SETTINGS))
@pytest.mark.parametrize('mode', MODES)
def test_host_core_equals_oracle_small_sizes(mode, setting):
    """Every (H, W) with both in {1..18, 31, 32, 33}: odd sizes (taps that are not 2x: 2/3 at 3,
    1 at 1), the crop of the T.81 planes, partial blocks and MCUs."""
    rng = np.random.default_rng(17)
    for H in SMALL:
        for W in SMALL:
            got, exp = both(rng, H, W, mode, **SETTINGS[setting])
            assert np.array_equal(got, exp), (H, W, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize('setting', sorted(SETTINGS))
@pytest.mark.parametrize('mode', MODES)
def test_host_core_equals_oracle_tile_edges(mode, setting):
    th, tw = tile()
    rng = np.random.default_rng(23)
    for H, W in ((th - 1, tw + 1), (th + 1, 2 * tw - 1), (2 * th + 1, tw + 1)):
        got, exp = both(rng, H, W, mode, **SETTINGS[setting])
        assert np.array_equal(got, exp), (H, W, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize('mode', MODES)
def test_comparison_is_not_all_saturated(mode):
    """The saturating setting reaches both ends of the byte range and still leaves a large
    share of interior bytes: equality above is not an equality of clipped constants."""
    got, exp = both(np.random.default_rng(0), 65, 130, mode, **SETTINGS['saturating'])
    assert (exp == 0).any() and (exp == 255).any()
    between = np.mean((exp > 0) & (exp < 255))
    print(mode, 'share at 0', np.mean(exp == 0), 'at 255', np.mean(exp == 255), 'between', between)
    assert between >= 0.30
    assert np.array_equal(got, exp)


@pytest.mark.parametrize('name', NAMES)
def test_host_core_equals_oracle_on_fixtures(name):
    from jds import codec
    data, cf = fixture(name)
    d = ir.decode(data)
    got = codec.host_jpeg_inverse(cf, d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
    assert np.array_equal(got, oracle_image(cf, d['H'], d['W'], d['mode'], d['qtables'], d['grids']))


def _window(d0, d1, n, src, xaxis):
    from jds import _abi
    out = (C.c_int32 * 4)()
    _abi.check(_abi.lib().jds_selftest_jpeg_window(d0, d1, n, src, int(xaxis), out))
    return tuple(out)


def test_window_holds_every_tap():
    """For every axis length 1..200 and every tile along it, the samples NumPy's tap table
    (oracle/cpu_ref.py:_linear_tab, rows clipped / columns clamped) reads lie inside the window
    jpeg_inv_window returns, and the window fits the kernel's array.  A tile's window is the
    product of a row interval and a column interval, each a function of its own axis alone, so
    every H on the row axis and every W on the column axis cover every H x W."""
    th, tw = tile()
    for xaxis, T in ((False, th), (True, tw)):
        for n in range(1, 201):
            src = -(-n // 2)
            s, _, _, _ = cpu_ref._linear_tab(n, src, clamp=xaxis)
            i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
            for d0 in range(0, n, T):
                d1 = min(d0 + T, n) - 1
                origin, extent, cap_rows, cap_cols = _window(d0, d1, n, src, xaxis)
                lo, hi = int(i0[d0:d1 + 1].min()), int(i1[d0:d1 + 1].max())
                assert origin <= lo and hi < origin + extent, (xaxis, n, d0, origin, extent, lo, hi)
                assert 0 <= origin and origin + extent <= src
                assert extent <= (cap_cols if xaxis else cap_rows), (xaxis, n, d0, extent)


def _info(H, W, mode, qt):
    from jds import codec
    return codec._jpeg_info_struct(H, W, mode, qt, ir.geometry(H, W, mode)[1])


@pytest.mark.parametrize('bad', [0, 256, 1.5])
def test_table_entries_outside_1_255_are_rejected(bad):
    from jds import _abi, codec
    cf, grids = planar(np.random.default_rng(1), 16, 16, '4:2:0')
    qt = QT.copy()
    qt[1, 0, 5] = bad
    with pytest.raises(ValueError, match=r'qtable\[1\]\[5\]'):
        codec.host_jpeg_inverse(cf, 16, 16, '4:2:0', qt, grids)
    # jds_jpeg_inverse_dev checks its arguments before it touches a device: no context needed
    st = _info(16, 16, '4:2:0', qt)
    with pytest.raises(ValueError, match=r'qtable\[1\]\[5\]'):
        _abi.check(_abi.lib().jds_jpeg_inverse_dev(None, C.byref(st), None, None, None))
    st = _info(16, 16, '4:2:0', QT)
    st.grid_cols[1] = 2          # not the T.81 grid of 16x16 4:2:0
    with pytest.raises(ValueError, match='T.81 geometry'):
        _abi.check(_abi.lib().jds_jpeg_inverse_dev(None, C.byref(st), None, None, None))
