"""CPU checks of the interleaved-scan decoder (no GPU): the parser
(jds_jpeg_parse), the host model of the decode (jds_selftest_jpegdec, the
kernels' shared core), the reference decoder / writer they are compared with
(tests/interleaved_ref.py) and the definition of the staged inverse."""
import glob
import io
import json
import os

import numpy as np
import pytest

import interleaved_ref as ir
import restart_ref as rr
from conftest import ROOT
from oracle import cpu_ref
from oracle import jpeg_entropy as je

GOLD = os.path.join(ROOT, 'tests', 'golden', 'jpeg_interleaved')
MANIFEST = json.load(open(os.path.join(GOLD, 'manifest.json')))
NAMES = sorted(MANIFEST['files'])
Q50 = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50)
QC = np.clip(Q50 * 2 + 3, 1, 255)   # a second, different table


def fixture(name):
    return open(os.path.join(GOLD, name + '.jpg'), 'rb').read(), np.load(os.path.join(GOLD, name + '.npy'))


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def written(H, W, mode, seed, ri=0, pad_dc=None, tq=(0, 1, 1)):
    rng = np.random.default_rng(seed)
    padded = ir.random_padded(rng, H, W, mode, pad_dc=pad_dc)
    qt = {0: Q50, 1: QC} if max(tq) else {0: Q50}
    data = ir.write(padded, H, W, mode, qt, tq=tq, ri=ri)
    return data, padded, ir.crop(padded, ir.geometry(H, W, mode)[1])


def test_manifest_covers_the_required_ground():
    f = MANIFEST['files']
    assert len(f) >= 8 and all(v['bytes'] < 100 * 1024 for v in f.values())
    assert any(v['max_code_length'] > 8 and v['args'].get('optimize') for v in f.values())
    assert f['p17x23_420']['padded_blocks'] > 0 and f['p33x35_422']['padded_blocks'] > 0
    assert any(v['restart_interval'] for v in f.values())


# ------------------------------------------------------ reference decoder --

@pytest.mark.parametrize('name', NAMES)
def test_reference_decoder_reproduces_the_scan_bytes(name):
    """writer(decoder(file).padded, file's tables) == the file's entropy-coded segment: the
    identity that makes the reference decoder trustworthy on foreign files."""
    data, exp = fixture(name)
    d = ir.decode(data)
    assert ir.entropy_segment(d['padded'], d['H'], d['W'], d['mode'], d['huff'], d['scan_tables'], d['ri']) == d['segment']
    assert np.array_equal(d['planar'], exp)
    # and the whole file from the writer decodes to the same grids
    again = ir.decode(ir.write(d['padded'], d['H'], d['W'], d['mode'], d['qt'], d['tq'], d['huff'],
                               d['scan_tables'], d['ri']))
    assert all(np.array_equal(a, b) for a, b in zip(again['padded'], d['padded']))


def test_reference_decoder_against_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(5)
    for (h, w), sub, kw in (((21, 37), 2, {}), ((16, 50), 1, {'optimize': True}), ((19, 19), 0, {}),
                            ((40, 40), 2, {'restart_marker_blocks': 2}), ((35, 33), 2, {'restart_marker_rows': 1})):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, 'JPEG', quality=60, subsampling=sub, **kw)
        d = ir.decode(buf.getvalue())
        assert ir.entropy_segment(d['padded'], h, w, d['mode'], d['huff'], d['scan_tables'], d['ri']) == d['segment']
        from jds import entropy
        assert np.array_equal(entropy.host_decode_jpeg(buf.getvalue(), 128)[0], d['planar'])


# ------------------------------------------------------------------ parser --

@pytest.mark.parametrize('name', NAMES)
def test_parse_fixture(name):
    from jds import entropy
    data, exp = fixture(name)
    m = MANIFEST['files'][name]
    ref = ir.decode(data)
    d = entropy.parse_jpeg(data)
    assert (d['H'], d['W'], d['mode']) == (m['H'], m['W'], m['mode'])
    assert d['interleaved'] and len(d['scans']) == 1
    assert [list(g) for g in d['grids']] == m['grids']
    assert [d['mcu']['rows'], d['mcu']['cols']] == m['mcu']
    assert d['mcu']['blocks'] == {'4:2:0': 6, '4:2:2': 4, '4:4:4': 3}[m['mode']]
    assert d['coeffs_needed'] == exp.size == 64 * sum(r * c for r, c in m['grids'])
    assert d['tq'] == m['tq'] and d['single_table'] == (len(set(m['tq'])) == 1)
    assert np.array_equal(d['qtables'], ref['qtables'])
    sc = d['scans'][0]
    assert sc['components'] == [1, 2, 3]
    assert list(zip(sc['dc_tables'], sc['ac_tables'])) == [tuple(t) for t in ref['scan_tables']]
    assert sc['restart_interval'] == m['restart_interval']
    assert data[sc['offset']:sc['offset'] + sc['length']] == ref['segment']
    for (tc, th), (bits, vals) in ref['huff'].items():
        assert d['huffman'][('dc', 'ac')[tc] + str(th)] == (bits, vals)
    try:
        rr_ok = rr.counts(m['H'], m['W'], m['mode'])[1] == m['grids'][1][0] * m['grids'][1][1] \
            and min(m['H'] // (2 if m['mode'] == '4:2:0' else 1), m['W'] // (1 if m['mode'] == '4:4:4' else 2)) >= 1
    except ZeroDivisionError:
        rr_ok = False
    assert d['reference_grid'] == rr_ok
    if name == 'p17x23_420':
        assert not d['reference_grid']


@pytest.mark.parametrize('h,w,mode,ri', [(24, 40, '4:2:0', 0), (33, 47, '4:4:4', 0), (48, 40, '4:2:2', 3), (16, 16, '4:2:0', 64)])
def test_files_parse_jfif_accepts_parse_alike(h, w, mode, ri):
    from jds import entropy
    ny, nc = rr.counts(h, w, mode)
    cf = np.random.default_rng(h + w).integers(-20, 21, (ny + 2 * nc) * 64).astype(np.int16)
    data = rr.encode_jfif_rst(cf, h, w, mode, Q50, ri)[0] if ri else je.encode_jfif(cf, h, w, mode, Q50, ny, nc)[0]
    a, b = entropy.parse_jfif(data), entropy.parse_jpeg(data)
    assert not b['interleaved'] and b['reference_grid'] and b['single_table']
    assert [(s['offset'], s['length'], s['restart_interval']) for s in a['scans']] == \
        [(s['offset'], s['length'], s['restart_interval']) for s in b['scans']]
    assert [s['component'] for s in a['scans']] == [s['components'][0] for s in b['scans']]
    assert np.array_equal(a['qtable'], b['qtables'][0]) and a['coeffs_needed'] == b['coeffs_needed']
    for S in (64, 1024):
        assert np.array_equal(entropy.host_decode_jpeg(data, S)[0], cf)


def test_parse_rejections_by_name():
    from jds import entropy
    data, _ = fixture('p24x40_420')
    with pytest.raises(ValueError, match='two quantisation tables'):
        entropy.parse_jfif(data)     # existing behaviour, from the new side
    one_table = ir.decode(data)
    one_table = ir.write(one_table['padded'], 24, 40, '4:2:0', {0: Q50}, (0, 0, 0))
    with pytest.raises(ValueError, match='interleaved scan'):
        entropy.parse_jfif(one_table)
    sos = data.index(b'\xff\xda')
    # Ns = 2
    two = data[:sos] + b'\xff\xda\x00\x0a\x02\x01\x00\x02\x11\x00\x3f\x00' + data[sos + 14:]
    with pytest.raises(ValueError, match=r'Ns = 2'):
        entropy.parse_jpeg(two)
    sof = data.index(b'\xff\xc0')
    with pytest.raises(ValueError, match='progressive'):
        entropy.parse_jpeg(data[:sof + 1] + b'\xc2' + data[sof + 2:])
    gray = data[:sof] + b'\xff\xc0\x00\x0b\x08\x00\x18\x00\x28\x01\x01\x11\x00' + data[sof + 19:]
    with pytest.raises(ValueError, match='grayscale'):
        entropy.parse_jpeg(gray)
    dqt = data.index(b'\xff\xdb')
    with pytest.raises(ValueError, match='16-bit DQT'):
        entropy.parse_jpeg(data[:dqt + 4] + bytes([data[dqt + 4] | 0x10]) + data[dqt + 5:])
    # a mix of the two scan forms: an Ns = 1 scan after the interleaved one
    eoi = len(data) - 2
    with pytest.raises(ValueError, match='mix of interleaved'):
        entropy.parse_jpeg(data[:eoi] + je.sos(1) + b'\x00' + data[eoi:])
    with pytest.raises(ValueError, match='12-bit'):
        entropy.parse_jpeg(data[:sof + 4] + b'\x0c' + data[sof + 5:])
    for cut in (3, sof + 6, sos + 5, len(data) - 2):
        with pytest.raises(ValueError):
            entropy.parse_jpeg(data[:cut])


# -------------------------------------------------------------- host model --

@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('S', [64, 128, 1024])
def test_host_model_fixture(name, S):
    from jds import entropy
    data, exp = fixture(name)
    cf, rounds = entropy.host_decode_jpeg(data, S)
    assert np.array_equal(cf, exp)
    sc = entropy.parse_jpeg(data)['scans'][0]
    nsub = -(-8 * sc['length'] // S)
    assert len(rounds) == 1 and (rounds[0] == 0 if sc['restart_interval'] else 1 <= rounds[0] <= nsub)


@pytest.mark.parametrize('h,w,mode', [(41, 50, '4:2:0'), (17, 23, '4:2:0'), (33, 35, '4:2:2'), (20, 28, '4:4:4')])
@pytest.mark.parametrize('S', [64, 128, 1024])
def test_host_model_writer_files(h, w, mode, S):
    from jds import entropy
    data, padded, exp = written(h, w, mode, 3 * h + w)
    assert mode == '4:4:4' or sum(p.shape[0] * p.shape[1] for p in padded) * 64 > exp.size     # padding blocks
    cf, rounds = entropy.host_decode_jpeg(data, S)
    assert np.array_equal(cf, exp)
    nsub = -(-8 * entropy.parse_jpeg(data)['scans'][0]['length'] // S)
    assert 1 <= rounds[0] <= nsub
    assert np.array_equal(ir.decode(data)['planar'], exp)


def test_dc_chain_runs_through_padding_blocks():
    """Padding blocks with DC +-1000: a decoder that leaves them out of the prediction, or
    stores them, gets the kept blocks' DCs wrong."""
    from jds import entropy
    data, padded, exp = written(17, 23, '4:2:0', 77, pad_dc=1000)
    assert np.abs(padded[0][:, :, 0]).max() == 1000      # (17x23 4:2:0 pads the luma grid, 3x3 to 4x4)
    for S in (64, 1024):
        cf, _ = entropy.host_decode_jpeg(data, S)
        assert np.array_equal(cf.reshape(-1, 64)[:, 0], exp.reshape(-1, 64)[:, 0])
        assert np.array_equal(cf, exp)
    data, padded, exp = written(17, 23, '4:2:0', 78, pad_dc=1000, ri=1)
    assert np.array_equal(entropy.host_decode_jpeg(data)[0], exp)


@pytest.mark.parametrize('h,w,mode,ri', [(40, 56, '4:2:0', 1), (40, 56, '4:2:0', 2), (40, 56, '4:2:0', 4), (33, 35, '4:2:2', 3),
                                        (160, 160, '4:2:0', 64), (20, 100, '4:4:4', 5)])
def test_host_model_restart(h, w, mode, ri):
    """Ri of 1 and 2 MCUs, one MCU row (56 wide 4:2:0: 4 MCUs), a last short interval, more
    than 8 intervals (RSTm wraps), and Ri * 6 above lane_max_blocks (the descriptor route)."""
    from jds import entropy
    data, padded, exp = written(h, w, mode, h + ri, ri=ri)
    d = entropy.parse_jpeg(data)
    nmcu = d['mcu']['rows'] * d['mcu']['cols']
    assert d['scans'][0]['restart_interval'] == ri
    if ri == 1:
        assert nmcu > 8      # RSTm wraps
    if (h, w, ri) == (40, 56, 4):
        assert d['mcu']['cols'] == ri
    for S in (64, 1024):
        cf, rounds = entropy.host_decode_jpeg(data, S)
        assert np.array_equal(cf, exp)
    lane_max = entropy.restart_info()[1]
    assert (rounds[0] > 0) == (ri * d['mcu']['blocks'] > lane_max)


def test_restart_marker_defects_are_caught():
    from jds import entropy
    data, _, _ = written(40, 56, '4:2:0', 9, ri=2)
    pos = [i for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(pos) == -(-12 // 2) - 1
    with pytest.raises(ValueError, match='restart markers where DRI'):
        entropy.parse_jpeg(data[:pos[-1]] + data[pos[-1] + 2:])                     # the last one removed
    swapped = bytearray(data)
    swapped[pos[1] + 1], swapped[pos[2] + 1] = swapped[pos[2] + 1], swapped[pos[1] + 1]
    with pytest.raises(ValueError, match='where RST'):
        entropy.parse_jpeg(bytes(swapped))                                          # out of order
    dri = data.index(b'\xff\xdd')
    with pytest.raises(ValueError, match='without a restart interval'):
        entropy.parse_jpeg(data[:dri] + data[dri + 6:])                             # markers, no DRI


def test_host_model_defects():
    from jds import entropy
    data, _ = fixture('p24x40_420')
    sc = entropy.parse_jpeg(data)['scans'][0]
    cut = data[:sc['offset'] + sc['length'] // 2] + data[sc['offset'] + sc['length']:]
    with pytest.raises(ValueError, match='defective scan data'):
        entropy.host_decode_jpeg(cut, 128)


def test_zero_file_variant_needs_wrong_slot_rounds():
    """The all-zero 4:2:0 file has 32-bit MCUs, so every slot-0 guess at S = 64 is right; with one
    AC coefficient in every Cb block the MCU length no longer divides S and guesses land in other
    slots: the model needs propagation rounds (the GPU test of the same files relies on it)."""
    from jds import entropy
    for variant, lo in ((False, 1), (True, 2)):
        data, exp = zero_file(variant)
        cf, rounds = entropy.host_decode_jpeg(data, 64)
        assert np.array_equal(cf, exp) and rounds[0] >= lo, rounds


def zero_file(variant, h=64, w=64):
    padded = [np.zeros(s + (64,), np.int64) for s in ir.padded_shapes(h, w, '4:2:0')]
    if variant:
        padded[1][:, :, 1] = 1
    return ir.write(padded, h, w, '4:2:0', {0: Q50, 1: QC}), ir.crop(padded, ir.geometry(h, w, '4:2:0')[1])


# ---------------------------------------------------------- staged inverse --

def oracle_image(planar, H, W, mode, qtables, grids):
    """decompress_jpeg's staged route in the oracle's terms: dequantize -> decode_blocks ->
    merge_blocks -> crop to the T.81 plane -> upsample_chroma -> ycbcr_to_rgb -> clip/astype."""
    hmax, vmax = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}[mode]
    blocks = np.asarray(planar, np.int16).reshape(-1, 8, 8)
    planes, b0 = [], 0
    for c, (gr, gc) in enumerate(grids):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        px = cpu_ref.decode_blocks(cpu_ref.dequantize(blocks[b0:b0 + gr * gc], qtables[c]))
        b0 += gr * gc
        planes.append(cpu_ref.merge_blocks(px, (8 * gr, 8 * gc))[:-(-H * vs // vmax), :-(-W * hs // hmax)])
    y, cb, cr = planes
    if mode != '4:4:4':
        cb, cr = cpu_ref.upsample_chroma(cb, cr, (H, W))
    return np.clip(cpu_ref.ycbcr_to_rgb(np.stack([y, cb, cr], axis=-1)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('name', NAMES)
def test_staged_inverse_definition(name):
    """Pins the expected images of the GPU test: shape, dtype, and that they are a decode of the
    file (close to Pillow's where Pillow is present; the two inverses differ by design)."""
    data, exp = fixture(name)
    d = ir.decode(data)
    img = oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
    assert img.shape == (d['H'], d['W'], 3) and img.dtype == np.uint8
    if MANIFEST['files'][name]['content'] == 'gray':
        assert np.all(img == 128)
    try:
        from PIL import Image
    except ImportError:
        return
    pil = np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).astype(int)
    diff = np.abs(pil - img)
    # reported, not asserted: libjpeg's integer IDCT and its chroma upsampling differ by design
    print(name, 'vs Pillow: max', diff.max(), 'mean', diff.mean())
