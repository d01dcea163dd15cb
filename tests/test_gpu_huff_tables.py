"""GPU checks of the Huffman decode core on hostile tables and 0xFF-dense scans
(tests/huff_hostile.py): bit-equality of jds_decode_jpeg / jds_decode_jfif with the coefficients
that were written, through both device byte sources (DecLdsSrc of k_dec_sync / k_dec_write,
RstRowSrc of k_dec_rst): every table family in one workgroup, the dense scans at the four byte
alignments of the scan's start (dec_stage's mis / o0) within one workgroup and across three,
both restart routes, three-scan files (the HdPlain instantiations, k_dec_dc), crossed table ids,
a batch whose files all carry different tables (tabs + 4 * file), and defective scans.  The
properties of the files themselves are asserted in tests/test_huff_tables_cpu.py."""
import numpy as np
import pytest

import huff_hostile as hh
import interleaved_ref as ir
from test_jpeg_interleaved_cpu import oracle_image

pytestmark = pytest.mark.gpu

# (family, stream, crossed table ids)
KINDS = [('ladder8', 'ff_dense', False), ('ladder8', 'ff_mixed', False), ('ladder16ff', 'ff_dense10', False),
         ('ladder16ff', 'ff_mixed10', False), ('ladder16', 'long_codes', False),
         ('gap', 'long_codes', False), ('flat8', 'sparse_random', False), ('random', 'sparse_random', False),
         ('random_open', 'sparse_random', False)]
KIND_IDS = ['-'.join(k[:2]) for k in KINDS]


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def groups_of(data):
    """(subsequences, workgroups) of a file's first scan."""
    from jds import entropy
    S, G = entropy.decode_info()
    n = entropy.parse_jpeg(data)['scans'][0]['length']
    return -(-8 * n // S), -(-8 * n // (S * G))


@pytest.mark.parametrize('mode', hh.MODES)
@pytest.mark.parametrize('family,strm,crossed', KINDS, ids=KIND_IDS)
def test_gpu_family_single_workgroup(family, strm, crossed, mode):
    from jds import entropy
    h, w = (25, 40) if strm == 'ff_dense10' else (40, 56)       # (416 bytes a block: 40x56 4:4:4 would be two workgroups)
    data, exp = hh.case(family, strm, h, w, mode, crossed=crossed)[:2]
    nsub, ngroups = groups_of(data)
    assert ngroups == 1
    d = entropy.decode_jpeg(data)
    assert d['coeffs'].dtype == np.int16 and np.array_equal(d['coeffs'], exp), np.flatnonzero(d['coeffs'] != exp)[:4]
    assert 1 <= d['rounds'] <= nsub


@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('family,strm,h,w', [('ladder8', 'ff_dense', 40, 56), ('ladder8', 'ff_mixed', 40, 56),
                                             ('ladder16ff', 'ff_dense10', 25, 40), ('ladder16ff', 'ff_mixed10', 40, 56),
                                             ('ladder8', 'ff_dense', 112, 112), ('ladder8', 'ff_mixed', 176, 176),
                                             ('ladder16ff', 'ff_dense10', 96, 96), ('ladder16ff', 'ff_mixed10', 128, 128)])
def test_gpu_ff_scans_at_every_alignment(family, strm, h, w, k):
    """The scan's first byte at each of the four residues mod 4, in one workgroup and in a scan of
    at least three (a workgroup's ragged start and its tail)."""
    from jds import entropy
    base, exp = hh.case(family, strm, h, w, '4:2:0')[:2]
    data = hh.shift(base, k)
    off = entropy.parse_jpeg(data)['scans'][0]['offset']
    assert off == hh.scans(base)[0][0] + 4 + k      # k = 0..3: the four residues
    nsub, ngroups = groups_of(data)
    assert ngroups >= 3 if h > 56 else ngroups == 1, (len(hh.scans(base)[0][1]), ngroups)
    d = entropy.decode_jpeg(data)
    assert np.array_equal(d['coeffs'], exp), (off % 4, np.flatnonzero(d['coeffs'] != exp)[:4])
    assert 1 <= d['rounds'] <= ngroups


@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('strm,family,ri', [('ff_dense', 'ladder8', 1), ('ff_dense10', 'ladder16ff', 2), ('long_codes', 'ladder16', 3),
                                            ('long_codes', 'gap', 5), ('ff_dense', 'ladder8', 22), ('ff_mixed10', 'ladder16ff', 22),
                                            ('long_codes', 'ladder16', 22)])
def test_gpu_restart_routes_hostile(strm, family, ri, k):
    """Lane route (RstRowSrc: intervals longer than its 128-byte row, so the row refills within
    an interval) and descriptor route (Ri * 6 blocks above the lane limit), a last short interval
    on both, the file at the four alignments."""
    from jds import entropy
    base, exp = hh.case(family, strm, 112, 112, '4:2:0', seed=4, ri=ri)[:2]
    data = hh.shift(base, k)
    d = entropy.parse_jpeg(data)
    nmcu, bpm = d['mcu']['rows'] * d['mcu']['cols'], d['mcu']['blocks']
    assert d['scans'][0]['restart_interval'] == ri and (ri == 1 or nmcu % ri) and d['scans'][0]['offset'] % 4 == \
        (hh.scans(base)[0][0] + k) % 4
    lens = [len(p) for p in hh.intervals(hh.scans(data)[0][1])]
    assert len(lens) == -(-nmcu // ri) and max(lens) > 128, max(lens)
    lane = ri * bpm <= entropy.restart_info()[1]
    assert lane == (ri != 22)
    out = entropy.decode_jpeg(data)
    assert np.array_equal(out['coeffs'], exp), np.flatnonzero(out['coeffs'] != exp)[:4]
    assert (out['rounds'] == 0) == lane


@pytest.mark.parametrize('ri', [0, 5])
@pytest.mark.parametrize('family,strm,crossed', KINDS + [('mixed', 'sparse_random', True)], ids=KIND_IDS + ['mixed-crossed'])
def test_gpu_three_scan_files_with_custom_tables(family, strm, crossed, ri):
    """decode_jfif (one quantisation table, the reference's grids) and decode_jpeg on the same
    file, and decode_jpeg on a file with T.81 grids decode_jfif does not take."""
    from jds import entropy
    data, exp = hh.case(family, strm, 40, 56, '4:2:0', seed=3, ri=ri, interleaved=False, crossed=crossed, one_qt=True)[:2]
    a = entropy.decode_jfif(data)
    assert np.array_equal(a['coeffs'], exp), np.flatnonzero(a['coeffs'] != exp)[:4]
    b = entropy.decode_jpeg(data)
    assert not b['interleaved'] and np.array_equal(b['coeffs'], exp)
    assert (a['rounds'] == 0) == (b['rounds'] == 0) == bool(ri)
    data, exp = hh.case(family, strm, 17, 23, '4:2:0', seed=3, ri=ri, interleaved=False, crossed=crossed)[:2]
    assert np.array_equal(entropy.decode_jpeg(data)['coeffs'], exp)


@pytest.mark.parametrize('mode', hh.MODES)
@pytest.mark.parametrize('ri', [0, 2])
def test_gpu_crossed_table_ids_four_families(mode, ri):
    """Y on DC 1 / AC 0, Cb on DC 0 / AC 1, Cr on DC 1 / AC 1, the four tables of four families."""
    from jds import entropy
    for family, strm in (('mixed', 'sparse_random'), ('random_open', 'sparse_random'), ('ladder16', 'long_codes')):
        data, exp = hh.case(family, strm, 41, 50, mode, seed=5, ri=ri, crossed=True)[:2]
        sc = entropy.parse_jpeg(data)['scans'][0]
        assert list(zip(sc['dc_tables'], sc['ac_tables'])) == list(hh.CROSSED)
        out = entropy.decode_jpeg(data)
        assert np.array_equal(out['coeffs'], exp), (family, np.flatnonzero(out['coeffs'] != exp)[:4])


def test_gpu_batch_of_different_tables():
    """Six files, each with tables of another family, mixed modes and sizes, one with restart
    intervals and one of three scans: every image equals the single-file call's and the oracle's
    image of the written coefficients.  With shared tables a wrong `tabs + 4 * file` would pass."""
    from jds import codec
    specs = [('ladder8', 'ff_mixed', 40, 56, '4:2:0', {}), ('ladder16', 'long_codes', 33, 35, '4:2:2', {}),
             ('gap', 'long_codes', 20, 28, '4:4:4', {}), ('flat8', 'sparse_random', 41, 50, '4:2:0', {'ri': 2}),
             ('random', 'sparse_random', 17, 23, '4:2:0', {'interleaved': False}),
             ('mixed', 'sparse_random', 24, 40, '4:2:2', {'crossed': True})]
    cases = [hh.case(f, s, h, w, m, seed=6, **kw) for f, s, h, w, m, kw in specs]
    files = [c[0] for c in cases]
    assert len({repr(sorted(c[3].items())) for c in cases}) == len(cases)      # no two files share their tables
    imgs = codec.jpeg_batch_to_rgb(files)
    for (f, s, h, w, m, kw), c, img in zip(specs, cases, imgs):
        qt = np.stack([hh.Q50, hh.QC, hh.QC])
        assert np.array_equal(img, codec.jpeg_to_rgb(c[0])), f
        assert np.array_equal(img, oracle_image(c[1], h, w, m, qt, ir.geometry(h, w, m)[1])), f


def test_gpu_defective_scans_with_hostile_tables():
    """Ordinary bounded decodes of bad data (a size-12 symbol from a 256-symbol table; the
    unassigned all-ones code of an incomplete table): a ValueError each, and the context decodes
    the next file."""
    from jds import entropy
    good, exp = hh.case('flat8', 'sparse_random', 24, 40, '4:2:0', seed=9)[:2]
    for kind, f in hh.defective_files().items():
        with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x'):
            entropy.decode_jpeg(f)
        assert np.array_equal(entropy.decode_jpeg(good)['coeffs'], exp), kind
