"""CPU checks of the lossless transcode (DESIGN.md "Transcode"; no GPU): the host model
(jds_selftest_jpeg_transcode / jds_selftest_jpeg_encode: the host decode model, then the writer
through the kernels' shared block lookup, predecessor rule, header splicer and table builder)
against the definition (tests/transcode_ref.py) and against Pillow (libjpeg), whose plain and
optimize=True files of one image are each other's transcodes byte for byte."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import huffopt_ref as hr
import interleaved_ref as ir
import transcode_cases as tc
import transcode_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (100, 75)]


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def host(data, optimize):
    from jds import entropy
    return entropy.host_transcode_jpeg(data, optimize)


# ------------------------------------------------------------ 1. Pillow oracle --

@pytest.mark.parametrize('mode', tc.MODES)
@pytest.mark.parametrize('h,w', SIZES)
def test_pillow_files_are_each_others_transcodes(h, w, mode):
    """Whole-file equality, host model == transcode_ref == Pillow, plain -> optimised and
    optimised -> plain, and the identity on an optimised file; with and without EXIF + ICC + COM."""
    for quality in (50, 92):
        for meta in (False, True):
            plain = tc.pillow(h, w, mode, quality, False, meta)
            opt = tc.pillow(h, w, mode, quality, True, meta)
            assert plain != opt
            assert tr.transcode(plain, True) == opt and tr.transcode(opt, False) == plain
            assert tr.transcode(opt, True) == opt
            assert host(plain, True) == opt, (quality, meta)
            assert host(opt, False) == plain, (quality, meta)
            assert host(opt, True) == opt, (quality, meta)
            if meta:
                assert tc.ICC in opt and tc.COMMENT in opt and tc.EXIF in opt


# ------------------------------------------------------------ 2. restart files --

@pytest.mark.parametrize('mode', tc.MODES)
@pytest.mark.parametrize('h,w', [(37, 53), (100, 75)])
@pytest.mark.parametrize('optimize', [False, True])
def test_pillow_restart_files_lose_their_intervals(h, w, mode, optimize):
    src = tc.pillow(h, w, mode, 50, False, True, restart_rows=1)
    assert b'\xff\xdd\x00\x04' in src and b'\xff\xd0' in src
    want = tc.pillow(h, w, mode, 50, optimize, True)
    assert tr.transcode(src, optimize) == want
    assert host(src, optimize) == want
    assert b'\xff\xdd\x00\x04' not in want


# ------------------------------------- 3. foreign padding and other table ids --

@pytest.mark.parametrize('case', tc.FOREIGN_CASES, ids=lambda c: f'{c[0]}x{c[1]}-{c[2]}-ri{c[6]}-{"3scan" if c[7] else "il"}-s{c[3]}')
@pytest.mark.parametrize('optimize', [False, True])
def test_foreign_files(case, optimize):
    src = tc.foreign(*case)
    want = tr.transcode(src, optimize)
    got = host(src, optimize)
    assert got == want
    d0, d1 = ir.decode(src), ir.decode(got)
    assert np.array_equal(d1['planar'], d0['planar'])
    assert d1['scan_tables'] == [(0, 0), (1, 1), (1, 1)] and d1['ri'] == 0 and d1['interleaved']
    assert d1['tq'] == d0['tq'] and np.array_equal(d1['qtables'], d0['qtables'])
    # libjpeg reads it, and sees the pixels of the input
    assert np.array_equal(tc.pixels(got), tc.pixels(src))


def test_padding_blocks_become_dummy_blocks():
    """The input's padding blocks carry content; the output's are AC zero with the DC of the
    preceding block of their component in scan order."""
    h, w, mode = 17, 33, '4:2:0'
    src = tc.foreign(h, w, mode, 1)
    d0, d1 = ir.decode(src), ir.decode(host(src, True))
    gr, gc = d1['grids'][0]
    y0, y1 = d0['padded'][0], d1['padded'][0]
    pad = np.ones(y1.shape[:2], bool)
    pad[:gr, :gc] = False
    assert np.any(y0[pad][:, 1:] != 0) and not np.any(y1[pad][:, 1:] != 0)
    last = 0
    for c, y, x in ir.mcu_order(h, w, mode):
        if c == 0:
            if pad[y, x]:
                assert y1[y, x, 0] == last
            last = int(y1[y, x, 0])


def test_own_three_scan_files():
    """This library's own profile (the reference writer's bytes, plain and optimised) in, one
    interleaved scan out."""
    from oracle import jpeg_entropy as je
    h, w, mode = 48, 64, '4:2:0'
    ny, nc = hr.counts(h, w, mode)
    cf = tc.random_coeffs(h, w, mode, 11)
    for src in (je.encode_jfif(cf, h, w, mode, tc.Q50, ny, nc)[0], hr.encode_jfif_opt(cf, h, w, mode, tc.Q50)[0]):
        for optimize in (False, True):
            got = host(src, optimize)
            assert got == tr.transcode(src, optimize)
            assert np.array_equal(ir.decode(got)['planar'], cf)


# ------------------------------------------------- 4. stuffing and long codes --

def test_stuffing_dense_scan():
    src = tc.pillow(64, 48, '4:2:0', 100, False, False, noise=True)
    scan = ir.decode(src)['segment']
    assert scan.count(b'\xff\x00') > 20           # the case cannot pass empty
    for optimize in (False, True):
        got = host(src, optimize)
        assert got == tr.transcode(src, optimize)
        assert ir.decode(got)['segment'].count(b'\xff\x00') > 0    # the writer stuffed, too
    assert host(src, True) == tc.pillow(64, 48, '4:2:0', 100, True, False, noise=True)


def test_histogram_that_drives_k3():
    from jds import entropy
    cf, info, hist = tc.k3_coeffs()
    padded = tr.dummy_padded(cf, info['H'], info['W'], info['mode'])
    h = tr.scan_histograms(padded, info['H'], info['W'], info['mode'])
    assert {s: int(c) for s, c in enumerate(h['ac0']) if c} == hist
    assert hr.unconstrained_length(h['ac0']) == 17          # K.3 runs on this scan's AC luma table
    prefix = tr.default_prefix(info['H'], info['W'], info['mode'], info['qtables'], info['tq'])
    got = entropy.host_encode_jpeg(cf, info, optimize=True)
    assert got == tr.write(cf, info['H'], info['W'], info['mode'], prefix, True)
    assert max(i + 1 for i, b in enumerate(hr.file_tables(got)['ac0'][0]) if b) == 16
    assert np.array_equal(ir.decode(got)['planar'], cf)


# ------------------------------------------------------------- 5. not codable --

def test_joined_intervals_not_codable():
    from jds import entropy
    src = tc.not_codable()
    cf, _ = entropy.host_decode_jpeg(src)                   # decodable: every interval starts from 0
    assert np.array_equal(cf, ir.decode(src)['planar'])
    for optimize in (False, True):
        with pytest.raises(tr.NotCodable):
            tr.transcode(src, optimize)
        with pytest.raises(ValueError, match='not baseline-codable'):
            host(src, optimize)


# ------------------------------------------- 6. encode_jpeg from coefficients --

@pytest.mark.parametrize('mode', tc.MODES)
@pytest.mark.parametrize('h,w', [(1, 1), (17, 33), (40, 24)])
def test_encode_from_raw_coefficients(h, w, mode):
    from jds import entropy
    cf = tc.random_coeffs(h, w, mode, 5 + h)
    info = tc.info_of(h, w, mode)
    prefix = tr.default_prefix(h, w, mode, info['qtables'], info['tq'])
    for optimize in (False, True):
        got = entropy.host_encode_jpeg(cf, info, optimize=optimize)
        assert got == tr.write(cf, h, w, mode, prefix, optimize)
        d = ir.decode(got)
        assert np.array_equal(d['planar'], cf) and d['tq'] == [0, 1, 1]
        assert np.array_equal(d['qtables'], info['qtables'])
        Image.open(io.BytesIO(got)).load()
    # a caller's prefix is placed as it is
    own = b'\xff\xfe\x00\x05abc' + prefix
    assert entropy.host_encode_jpeg(cf, info, prefix=own) == tr.write(cf, h, w, mode, own, False)


def test_encode_argument_errors():
    from jds import entropy
    h, w, mode = 17, 33, '4:2:0'
    cf = tc.random_coeffs(h, w, mode, 1)
    info = tc.info_of(h, w, mode)
    with pytest.raises(ValueError, match='coefficients'):
        entropy.host_encode_jpeg(cf[:-64], info)
    floor = dict(info, grids=[(3, 5), (1, 2), (1, 2)])      # the reference's floor-sized chroma grid
    with pytest.raises(ValueError, match='T.81'):
        entropy.host_encode_jpeg(np.zeros(64 * 19, np.int16), floor)
    bad_q = dict(info, qtables=np.stack([tc.Q50, tc.QC * 0, tc.QC]))
    with pytest.raises(ValueError, match='qtable'):
        entropy.host_encode_jpeg(cf, bad_q)


def test_rejected_files_keep_their_names():
    b = io.BytesIO()
    Image.fromarray(tc.image(16, 16)).save(b, 'JPEG', progressive=True)
    with pytest.raises(ValueError, match='progressive'):
        host(b.getvalue(), True)
    src = tc.pillow(17, 33, '4:2:0')
    with pytest.raises(ValueError):
        host(src[:len(src) // 2], True)


# ------------------------------------------------------------- 7. sanitizers --

def test_splicer_and_parser_under_sanitizers(tmp_path):
    """tools/jpeg_splice_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: the header splicer and the parser over files truncated at
    every byte, segment lengths past the end and hostile DHT segments."""
    cxx = next((c for c in (shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/lib/llvm/bin/clang++')
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'jpeg_splice_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'jpeg_splice_san.cpp'), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'ok' in r.stdout
