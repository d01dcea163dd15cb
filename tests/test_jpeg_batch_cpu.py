"""CPU checks of the batch of foreign files (no GPU): the layout (jds_jpeg_batch_layout) and the
host model of the whole batch (jds_selftest_jpeg_batch: the layout, the host decode model per
file, the host model of the batch inverse with the same tile map and per-image records).  The
yardsticks are the single-file host core (jds_selftest_jpegdec + jds_selftest_jpeg_inverse) and
the definition of the staged inverse (test_jpeg_interleaved_cpu.oracle_image)."""
import re

import numpy as np
import pytest

import interleaved_ref as ir
import restart_ref as rr
from oracle import jpeg_entropy as je
from test_jpeg_interleaved_cpu import NAMES, Q50, QC, fixture, oracle_image, written

Q2 = np.clip(QC + 7, 1, 255)
MODES = ['4:2:0', '4:4:4', '4:2:2']


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def sizes():
    """test_gpu_jpeg_rgb._sizes(): the nine tile-edge sizes."""
    from jds import codec
    th, tw = codec.jpeg_inverse_info()
    return [(1, 1), (1, 17), (2, 3), (7, 9), (15, 17), (th - 1, tw + 1), (th + 1, 2 * tw - 1), (2 * th + 1, tw + 1),
            (185, 199)]


def three_table_file(h, w, mode, seed):
    """test_gpu_jpeg_rgb.three_table_file's recipe: three distinct tables, coefficients that
    saturate both ends."""
    rng = np.random.default_rng(seed)
    padded = ir.random_padded(rng, h, w, mode, amp=300, density=0.9)
    grids = ir.geometry(h, w, mode)[1]
    data = ir.write(padded, h, w, mode, {0: Q50, 1: QC, 2: Q2}, tq=(0, 1, 2))
    return data, ir.crop(padded, grids), np.stack([Q50, QC, Q2]), grids


def single_host(data):
    """The single-file host core: (image, coefficients)."""
    from jds import codec, entropy
    d = entropy.parse_jpeg(data)
    cf, _ = entropy.host_decode_jpeg(data)
    return codec.host_jpeg_inverse(cf, d['H'], d['W'], d['mode'], d['qtables'], d['grids']), cf


def image_of(rgb, it):
    o = it['rgb_off']
    return rgb[o:o + it['H'] * it['W'] * 3].reshape(it['H'], it['W'], 3)


def coeffs_of(cf, it):
    return cf[it['coef_off']:it['coef_off'] + it['coeffs_needed']]


def check_layout(items, rgb_bytes, coef_entries):
    """Offsets are multiples of 256, regions disjoint and in order, the totals the sum of the
    parts (an image's part is its size rounded up to 256), failing files take no space."""
    ro = co = 0
    for it in items:
        if it['rc'] != 0:
            assert it['rgb_off'] == -1 and it['coef_off'] == -1 and it['coeffs_needed'] == 0
            continue
        assert it['rgb_off'] % 256 == 0 and it['rgb_off'] == ro and it['coef_off'] == co
        ro += -(-it['H'] * it['W'] * 3 // 256) * 256
        co += it['coeffs_needed']
    assert (rgb_bytes, coef_entries) == (ro, co)


def gaps_untouched(rgb, items):
    """host_jpeg_batch pre-fills the output with 0xA5: the bytes between an image's end and the
    next multiple of 256 keep it."""
    for it in items:
        if it['rc'] == 0:
            end = it['rgb_off'] + it['H'] * it['W'] * 3
            assert np.all(rgb[end:-(-end // 256) * 256] == 0xA5)


@pytest.mark.parametrize('order', ['manifest', 'shuffled'])
def test_fixture_batch(order):
    from jds import codec
    names = list(NAMES)
    assert len(names) >= 8
    if order == 'shuffled':
        names = [names[i] for i in np.random.default_rng(5).permutation(len(names))]
    files = [fixture(n) for n in names]
    rgb, cf, items = codec.host_jpeg_batch([f[0] for f in files])
    lay, rb, ce = codec.jpeg_batch_layout([f[0] for f in files])
    assert lay == [dict(it, status=0) for it in items] and rb == rgb.size and ce == cf.size
    check_layout(items, rb, ce)
    gaps_untouched(rgb, items)
    for (data, exp), it in zip(files, items):
        d = ir.decode(data)
        assert (it['rc'], it['status'], it['H'], it['W'], it['mode']) == (0, 0, d['H'], d['W'], d['mode'])
        assert np.array_equal(coeffs_of(cf, it), exp)
        assert np.array_equal(image_of(rgb, it), oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids']))


def tile_edge_batch():
    """The nine sizes in all three modes, ordered so that modes alternate (420, 444, 422, 420, ..)."""
    out = []
    for si, (h, w) in enumerate(sizes()):
        for mode in MODES:
            out.append((h, w, mode) + three_table_file(h, w, mode, 100 * si + len(mode) + h))
    return out


def test_tile_edge_batch_alternating_modes():
    from jds import codec
    batch = tile_edge_batch()
    assert [b[2] for b in batch[:4]] == ['4:2:0', '4:4:4', '4:2:2', '4:2:0'] and len(batch) == 27
    rgb, cf, items = codec.host_jpeg_batch([b[3] for b in batch])
    check_layout(items, rgb.size, cf.size)
    gaps_untouched(rgb, items)
    for (h, w, mode, data, exp, qt, grids), it in zip(batch, items):
        img, c1 = single_host(data)
        assert (it['H'], it['W'], it['mode'], it['status']) == (h, w, mode, 0)
        assert np.array_equal(coeffs_of(cf, it), c1) and np.array_equal(c1, exp)
        assert np.array_equal(image_of(rgb, it), img), (h, w, mode)


def test_small_counts_and_repeats():
    from jds import codec
    rgb, cf, items = codec.host_jpeg_batch([])
    assert rgb.size == 0 and cf.size == 0 and items == []
    assert codec.jpeg_batch_layout([]) == ([], 0, 0)
    data, exp = fixture('p33x35_422')
    img, _ = single_host(data)
    rgb, cf, items = codec.host_jpeg_batch([data])
    assert items[0]['rgb_off'] == 0 and np.array_equal(image_of(rgb, items[0]), img) and np.array_equal(cf, exp)
    rgb, cf, items = codec.host_jpeg_batch([data, data])
    check_layout(items, rgb.size, cf.size)
    assert items[1]['rgb_off'] == -(-33 * 35 * 3 // 256) * 256 and items[1]['coef_off'] == exp.size
    for it in items:
        assert np.array_equal(image_of(rgb, it), img) and np.array_equal(coeffs_of(cf, it), exp)


def _single_parse_rc(data):
    import ctypes as C
    from jds import _abi
    a = np.frombuffer(data, np.uint8)
    return _abi.lib().jds_jpeg_parse(a.ctypes.data, a.size, C.byref(_abi.JpegInfo()))


@pytest.mark.parametrize('case', ['not_a_jpeg', 'cut_in_sof'])
def test_item_that_does_not_parse(case):
    from jds import codec, _abi
    good0, good1 = fixture('p24x40_420')[0], fixture('p33x35_422')[0]
    bad = b'not a jpeg' if case == 'not_a_jpeg' else good0[:good0.index(b'\xff\xc0') + 6]
    rc = _single_parse_rc(bad)
    assert rc != 0
    rgb, cf, items = codec.host_jpeg_batch([good0, bad, good1])
    assert items[1]['rc'] == rc and items[0]['rc'] == items[2]['rc'] == 0
    assert _abi.lib().jds_last_error().decode().startswith('file 1: ')
    check_layout(items, rgb.size, cf.size)
    assert items[2]['rgb_off'] == -(-24 * 40 * 3 // 256) * 256      # the bad file takes no space
    for data, it in ((good0, items[0]), (good1, items[2])):
        img, c1 = single_host(data)
        assert np.array_equal(image_of(rgb, it), img) and np.array_equal(coeffs_of(cf, it), c1)


def _rejected_by_reference(data):
    try:
        ir.decode(data)
    except (AssertionError, IndexError, KeyError):
        return True
    return False


def flipped(data):
    """The first bit from the middle of the scan on whose flip the reference decoder fails (bytes
    that are or neighbour an 0xFF are left alone): test_gpu_jpeg_rgb._defects' construction."""
    from jds import entropy
    sc = entropy.parse_jpeg(data)['scans'][0]
    a, n = sc['offset'], sc['length']
    for bit in range(8 * (a + n // 2), 8 * (a + n - 2)):
        i, m = bit >> 3, 0x80 >> (bit & 7)
        if 0xFF in data[i - 1:i + 2] or data[i] ^ m == 0xFF:
            continue
        f = data[:i] + bytes([data[i] ^ m]) + data[i + 1:]
        if _rejected_by_reference(f):
            return f
    raise AssertionError('no rejected flip')


def host_single_status(data):
    """The status word the single host call reports for a defective file."""
    from jds import entropy
    with pytest.raises(ValueError, match='defective scan data') as e:
        entropy.host_decode_jpeg(data)
    return int(re.search(r'status 0x([0-9a-f]+)', str(e.value)).group(1), 16)


def test_defective_scan_in_the_middle():
    from jds import codec
    good0, good1 = fixture('p33x35_422')[0], fixture('p31x45_420_q95_opt')[0]
    bad = flipped(fixture('p24x40_420')[0])
    st = host_single_status(bad)
    assert st != 0
    rgb, cf, items = codec.host_jpeg_batch([good0, bad, good1])
    check_layout(items, rgb.size, cf.size)
    gaps_untouched(rgb, items)
    assert [it['rc'] for it in items] == [0, 0, 0] and [it['status'] for it in items] == [0, st, 0]
    assert items[1]['coeffs_needed'] > 0 and np.all(image_of(rgb, items[1]) == 0)
    for data, it in ((good0, items[0]), (good1, items[2])):
        img, c1 = single_host(data)
        assert np.array_equal(image_of(rgb, it), img) and np.array_equal(coeffs_of(cf, it), c1)


def test_three_scan_own_files_mixed_with_interleaved():
    from jds import codec
    h, w, mode = 40, 56, '4:2:2'
    ny, nc = rr.counts(h, w, mode)
    own_cf = np.random.default_rng(4).integers(-30, 31, (ny + 2 * nc) * 64).astype(np.int16)
    own = je.encode_jfif(own_cf, h, w, mode, Q50, ny, nc)[0]
    own_rst = rr.encode_jfif_rst(own_cf, h, w, mode, Q50, 7)[0]
    il = [fixture('p24x40_420')[0], written(41, 50, '4:2:0', 3)[0], written(40, 56, '4:2:0', 44, ri=4)[0]]
    files = [il[0], own, il[1], own_rst, il[2]]
    rgb, cf, items = codec.host_jpeg_batch(files)
    check_layout(items, rgb.size, cf.size)
    assert [it['interleaved'] for it in items] == [True, False, True, False, True]
    for data, it in zip(files, items):
        img, c1 = single_host(data)
        assert it['status'] == 0 and np.array_equal(coeffs_of(cf, it), c1)
        assert np.array_equal(image_of(rgb, it), img)
    assert np.array_equal(coeffs_of(cf, items[1]), own_cf) and np.array_equal(coeffs_of(cf, items[3]), own_cf)
