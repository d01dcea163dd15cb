"""Rows of the tiled 8x8 inverse's 4:2:0 tiles (CPU, no GPU).

k_inv_fast and k_inv2 start their 64-row tiles 8 luma rows above 64 ty when
that adds no tile row (csrc/jds_internal.hpp inv_tile_yoff): the 34 chroma
sample rows a tile's bilinear upsample reads then come from five block rows
instead of six.  jds_selftest_inv_rows reports the geometry the kernels use
(csrc/jds_inv_common.hpp InvRows).  Checked here against cv2's INTER_LINEAR
row taps restated independently: the tile rows partition the luma rows, and
every chroma sample row a tile's luma rows read is computed into its window
exactly once."""
import ctypes as C
import math

import pytest

HEIGHTS = [2, 8, 16, 48, 54, 56, 58, 64, 66, 72, 118, 120, 122, 128, 184, 192, 248, 1072, 1080, 1088, 2160]
EXPECT_YOFF = {56: 8, 64: 0, 72: 8, 120: 8, 128: 0, 1080: 8, 2160: 8}


@pytest.fixture(scope='module')
def L():
    from jds import _abi
    return _abi.lib()


def _rows(L, mode, H, ty):
    out = (C.c_int32 * 8)()
    need = (C.c_uint8 * 64)()
    assert L.jds_selftest_inv_rows(mode, H, ty, out, need) == 0
    keys = ('yoff', 'tile_rows', 'y0', 'nrows', 'cby0', 'ncbr', 'cwy0', 'cwr')
    d = dict(zip(keys, out))
    d['need'] = [[bool(need[8 * i + r]) for r in range(8)] for i in range(d['ncbr'])]
    return d


@pytest.mark.parametrize('H', HEIGHTS)
def test_offset_never_adds_a_tile_row_and_rows_partition(L, H):
    t0 = _rows(L, 2, H, 0)
    aligned = math.ceil(H / 64)
    assert t0['tile_rows'] == aligned
    assert t0['yoff'] == (8 if math.ceil((H + 8) / 64) == aligned else 0)
    if H in EXPECT_YOFF:
        assert t0['yoff'] == EXPECT_YOFF[H]
    owner = [0] * H
    for ty in range(t0['tile_rows']):
        t = _rows(L, 2, H, ty)
        assert t['yoff'] == t0['yoff'] and t['nrows'] == 64 and t['y0'] == 64 * ty - t['yoff']
        for y in range(max(t['y0'], 0), min(t['y0'] + t['nrows'], H)):
            owner[y] += 1
    assert owner == [1] * H


def test_1080p_and_4k_tile_rows():
    assert math.ceil(1080 / 64) == math.ceil(1088 / 64) == 17
    assert math.ceil(2160 / 64) == math.ceil(2168 / 64) == 34


def _cv2_rows(y, hc):
    """cv2 INTER_LINEAR at scale 1/2: the two source rows of destination row y, clamped."""
    s0 = math.floor((y + 0.5) * 0.5 - 0.5)
    return {min(max(s0, 0), hc - 1), min(max(s0 + 1, 0), hc - 1)}


@pytest.mark.parametrize('H', HEIGHTS)
def test_window_holds_every_row_the_upsample_reads_once(L, H):
    hc = H // 2
    ncy = (hc + 7) // 8
    t0 = _rows(L, 2, H, 0)
    for ty in range(t0['tile_rows']):
        t = _rows(L, 2, H, ty)
        assert t['ncbr'] == (5 if t['yoff'] else 6) and t['cwr'] == 34
        have = []
        for i in range(t['ncbr']):
            by = t['cby0'] + i
            if not 0 <= by < ncy:
                continue  # no such block row: the kernels skip it
            for r in range(8):
                if t['need'][i][r]:
                    have.append(by * 8 + r)
        assert len(have) == len(set(have)), (ty, have)
        assert all(t['cwy0'] <= s < t['cwy0'] + t['cwr'] for s in have), (ty, have)  # inside the LDS window
        want = set()
        for y in range(max(t['y0'], 0), min(t['y0'] + t['nrows'], H)):
            want |= _cv2_rows(y, hc)
        assert want <= set(have), (ty, sorted(want - set(have)))
        if t['yoff']:  # five rows of the top and bottom block rows, all of the three between
            assert [sum(n) for n in t['need']] == [5, 8, 8, 8, 5]
            assert t['need'][0] == [False] * 3 + [True] * 5 and t['need'][4] == [True] * 5 + [False] * 3
        else:
            assert [sum(n) for n in t['need']] == [1, 8, 8, 8, 8, 1]


@pytest.mark.parametrize('mode', [0, 1])
def test_other_subsamplings_keep_aligned_tiles(L, mode):
    for H in (56, 120, 1080):
        t = _rows(L, mode, H, 1)
        assert t['yoff'] == 0 and t['y0'] == t['nrows'] == 32 and t['cwy0'] == 32 and t['cwr'] == 32
        assert all(all(n) for n in t['need'])
