"""CPU checks of the Huffman decode core (csrc/jds_huffdec.hpp: hd_build, hd_window, hd_run) on
hostile tables and 0xFF-dense scans (tests/huff_hostile.py), no GPU: the host model
(jds_selftest_jpegdec / jds_selftest_huffdec, the kernels' shared core) and the reference decoder
(tests/interleaved_ref.py) against the coefficients that were written; hd_build's edge cases
through the parser; defective scans with hostile tables; and tools/hd_window_check.cpp, the
stand-alone comparison of hd_window / hd_run with a naive byte walk, built with
AddressSanitizer / UBSan.  The coverage the files claim (0xFF per five-byte window, code lengths
in use, scan alignments, interval lengths) is asserted here on the written files."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import huff_hostile as hh
import interleaved_ref as ir
from conftest import ROOT

SIZES = [(17, 23, '4:2:0'), (33, 35, '4:2:2'), (20, 28, '4:4:4')]
# (family, stream, crossed table ids)
KINDS = [('ladder8', 'ff_dense', False), ('ladder8', 'ff_mixed', False), ('ladder16ff', 'ff_dense10', False),
         ('ladder16ff', 'ff_mixed10', True), ('ladder16', 'long_codes', False),
         ('gap', 'long_codes', False), ('flat8', 'sparse_random', False), ('random', 'sparse_random', False),
         ('random_open', 'sparse_random', True), ('mixed', 'sparse_random', True), ('ladder16', 'long_codes', True)]
KIND_IDS = ['-'.join((f, s) + (('crossed',) if x else ())) for f, s, x in KINDS]


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


def padding_blocks(padded, exp):
    return sum(p.shape[0] * p.shape[1] for p in padded) * 64 - exp.size


# ---------------------------------------------------------------- the tables --

def test_families_satisfy_kraft_and_hold_what_they_claim():
    for name, f in hh.FAMILIES.items():
        for cls in (0, 1):
            bits, vals = f(cls)
            ok, complete = hh.kraft_ok(bits)
            assert ok and complete == (name not in ('gap', 'random_open')), (name, cls)
            assert set(range(12) if cls == 0 else ()) <= set(vals) or name == 'ladder8'
    assert hh.ladder8(1)[1][-1] == 0x08 and hh.ladder8(0)[1][-1] == 8          # the all-ones 8-bit code
    assert hh.ladder16(1)[1][-3:] == [0x11, 0x01, 0x00]                         # 15, 16, 16 (all ones) bits
    assert all(b == 0 for b in hh.GAP_BITS[8:12]) and all(hh.GAP_BITS[12:])
    assert sum(hh.FLAT8_BITS) == 256 and sorted(hh.flat8(1)[1]) == list(range(256))
    assert any(b for b in hh.random_table(1, 101 + 1)[0][12:])                  # random: codes beyond 12 bits
    assert not hh.kraft_ok([2, 1] + [0] * 14)[0] and not hh.kraft_ok([1] * 7 + [3] + [0] * 8)[0]


# ------------------------------------------- host model against the reference --

@pytest.mark.parametrize('h,w,mode', SIZES)
@pytest.mark.parametrize('family,strm,crossed', KINDS, ids=KIND_IDS)
def test_host_model_hostile_tables(family, strm, crossed, h, w, mode):
    from jds import entropy
    data, exp, padded, huff, st = hh.case(family, strm, h, w, mode, crossed=crossed)
    assert mode == '4:4:4' or padding_blocks(padded, exp) > 0
    d = entropy.parse_jpeg(data)
    assert d['interleaved'] and list(zip(d['scans'][0]['dc_tables'], d['scans'][0]['ac_tables'])) == list(st)
    for (tc, th), (bits, vals) in huff.items():
        assert d['huffman'][('dc', 'ac')[tc] + str(th)] == (bits, vals)
    assert np.array_equal(ir.decode(data)['planar'], exp)         # the reference is sound on these tables
    nbits = 8 * d['scans'][0]['length']
    for S in (64, 128, 1024):
        cf, rounds = entropy.host_decode_jpeg(data, S)
        assert np.array_equal(cf, exp), (S, np.flatnonzero(cf != exp)[:4])
        assert 1 <= rounds[0] <= -(-nbits // S)


@pytest.mark.parametrize('family,strm,crossed', KINDS, ids=KIND_IDS)
def test_host_model_hostile_restart_routes(family, strm, crossed):
    """Lane route (Ri * blocks per MCU <= the lane limit) and descriptor route, a last short
    interval on both."""
    from jds import entropy
    lane_max = entropy.restart_info()[1]
    for h, w, mode, ri in ((40, 56, '4:2:0', 5), (33, 35, '4:2:2', 4), (56, 64, '4:4:4', lane_max // 3 + 1)):
        data, exp, padded, _, _ = hh.case(family, strm, h, w, mode, seed=2, ri=ri, crossed=crossed)
        d = entropy.parse_jpeg(data)
        nmcu, bpm = d['mcu']['rows'] * d['mcu']['cols'], d['mcu']['blocks']
        assert d['scans'][0]['restart_interval'] == ri and nmcu % ri and nmcu > ri
        lane = ri * bpm <= lane_max
        assert lane == (mode != '4:4:4')
        assert np.array_equal(ir.decode(data)['planar'], exp)
        for S in (64, 1024):
            cf, rounds = entropy.host_decode_jpeg(data, S)
            assert np.array_equal(cf, exp), (h, w, mode, ri, S)
            assert (rounds[0] == 0) == lane


@pytest.mark.parametrize('family,strm,crossed', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('ri', [0, 5])
def test_host_model_three_scan_files(family, strm, crossed, ri):
    """Non-interleaved files with the file's own tables: through host_decode_jpeg always, and
    through host_decode_jfif where the geometry and the one quantisation table allow it."""
    from jds import entropy
    for h, w, mode, one_qt in ((40, 56, '4:2:0', True), (17, 23, '4:2:0', False), (33, 35, '4:2:2', True)):
        data, exp, _, _, st = hh.case(family, strm, h, w, mode, seed=3, ri=ri, interleaved=False, crossed=crossed,
                                      one_qt=one_qt)
        d = entropy.parse_jpeg(data)
        assert not d['interleaved'] and len(d['scans']) == 3
        assert [(s['dc_tables'][0], s['ac_tables'][0]) for s in d['scans']] == list(st)
        assert np.array_equal(ir.decode(data)['planar'], exp)
        for S in (64, 128, 1024):
            assert np.array_equal(entropy.host_decode_jpeg(data, S)[0], exp), (h, w, mode, S)
        if (h, w) == (40, 56):
            assert d['reference_grid'] and d['single_table']
            for S in (64, 1024):
                assert np.array_equal(entropy.host_decode_jfif(data, S)[0], exp), S
        elif (h, w) == (17, 23):
            assert not d['reference_grid']
            with pytest.raises(ValueError):
                entropy.parse_jfif(data)


# ------------------------------------------------------- what the files reach --

def test_ff_dense_is_dense_and_ff_mixed_reaches_every_window():
    """ff_dense: half of the stuffed bytes are 0xFF (all data bytes but the DC's), so nearly every
    window of five data bytes holds five (hd_window's byte walk).  ff_mixed: every count from 0
    to 5 occurs (no squeeze, each of its three steps, and the walk)."""
    for family, strm in (('ladder8', 'ff_dense'), ('ladder16ff', 'ff_dense10')):
        for mode in hh.MODES:
            data = hh.case(family, strm, 25, 40, mode)[0]
            seg = hh.scans(data)[0][1]
            n_ff, h = seg.count(b'\xff'), hh.ff_window_histogram(seg)
            assert seg.count(b'\xff\x00') == n_ff and 2 * n_ff > len(seg) - len(seg) // 50, (n_ff, len(seg))
            assert h[5] > 0.95 * h.sum() and h[4] > 0
    for family, strm, big in (('ladder8', 'ff_mixed', (176, 176, '4:2:0')), ('ladder16ff', 'ff_mixed10', (128, 128, '4:2:0'))):
        for h_, w_, mode in SIZES + [(40, 56, '4:2:0'), big]:
            data = hh.case(family, strm, h_, w_, mode)[0]
            h = hh.ff_window_histogram(hh.scans(data)[0][1])
            assert h.shape == (6,) and np.all(h > 0), (h_, w_, mode, h)


def test_dense10_symbols_span_five_data_bytes():
    """What ff_dense cannot reach: a ladder8 symbol is at most 16 bits, three data bytes at
    any bit offset.  ff_dense10's AC symbols are 26 bits (16-bit code, ten magnitude bits), its
    DC symbols 27, all of them 1-bits, and they start at every bit offset: hd_run needs the
    window's five data bytes and the stuffing counts of the first four."""
    h, w, mode = 25, 40, '4:2:0'
    _, _, padded, huff, st = hh.case('ladder16ff', 'ff_dense10', h, w, mode)
    codes = {k: hh.je.huffman_codes(t) for k, t in huff.items()}
    bit, offs, lens = 0, set(), set()
    for key, sym, mag, mlen in hh.il_entries(padded, h, w, mode, st):
        n = codes[key][sym][1] + mlen
        offs.add(bit & 7)
        lens.add(n)
        bit += n
    assert offs == set(range(8)) and lens == {26, 27}
    _, _, padded, huff, st = hh.case('ladder8', 'ff_dense', h, w, mode)
    codes = {k: hh.je.huffman_codes(t) for k, t in huff.items()}
    assert {codes[key][sym][1] + mlen for key, sym, _, mlen in hh.il_entries(padded, h, w, mode, st)} == {16}


def test_long_code_lengths_in_use():
    """gap and ladder16: every length 13..16 occurs among the AC codes (and the DC codes) of the
    stream, and none of 9..12 with gap; the all-ones 16-bit code of ladder16 is EOB."""
    for family in ('gap', 'ladder16'):
        for h, w, mode in SIZES + [(40, 56, '4:2:0')]:
            _, _, padded, huff, st = hh.case(family, 'long_codes', h, w, mode)
            used = hh.code_lengths_used(hh.il_entries(padded, h, w, mode, st), huff)
            for key in ((1, 0), (1, 1)):
                assert {13, 14, 15, 16} <= used[key], (family, h, w, mode, key, used[key])
            assert {13, 14, 15, 16} <= used[(0, 0)] | used[(0, 1)]
            if family == 'gap':
                assert not any(9 <= l <= 12 for v in used.values() for l in v)


def test_shift_covers_the_four_alignments():
    from jds import entropy
    data, exp = hh.case('ladder8', 'ff_dense', 40, 56, '4:2:0')[:2]
    offs = []
    for k in range(4):
        f = hh.shift(data, k)
        sc = entropy.parse_jpeg(f)['scans'][0]
        assert sc['offset'] == hh.scans(f)[0][0] == hh.scans(data)[0][0] + 4 + k
        assert f[sc['offset']:sc['offset'] + sc['length']] == hh.scans(data)[0][1]
        offs.append(sc['offset'])
        assert np.array_equal(entropy.host_decode_jpeg(f, 128)[0], exp)
        assert np.array_equal(ir.decode(f)['planar'], exp)
    assert sorted(o % 4 for o in offs) == [0, 1, 2, 3], offs


# ------------------------------------------------------------------ hd_build --

def _with_table(key, table):
    huff = dict(ir.STD_HUFF)
    huff[key] = table
    return ir.headers(16, 16, '4:4:4', {0: hh.Q50}, (0, 0, 0), huff) + ir.sos3(ir.STD_SCAN_TABLES) + b'\x00\xff\xd9'


@pytest.mark.parametrize('key', [(0, 1), (1, 0)])
def test_hd_build_edges_through_the_parser(key):
    from jds import entropy
    name = ('dc', 'ac')[key[0]] + str(key[1])
    for table in (hh.ladder8(key[0]), hh.ladder16(key[0]), hh.flat8(key[0])):      # complete; 256 symbols
        assert hh.kraft_ok(table[0]) == (True, True)
        assert entropy.parse_jpeg(_with_table(key, table))['huffman'][name] == table
    assert len(hh.flat8(key[0])[1]) == 256
    for bits in ([2, 1] + [0] * 14, [1] * 7 + [3] + [0] * 8, [1] * 15 + [3], [1] * 8 + [3] + [0] * 7):
        assert not hh.kraft_ok(bits)[0]
        with pytest.raises(ValueError, match='over-subscribe the code space'):
            entropy.parse_jpeg(_with_table(key, (bits, list(range(sum(bits))))))
    bits257 = [0] * 7 + [255, 2] + [0] * 7          # a complete code of 257 symbols
    assert hh.kraft_ok(bits257) == (True, True)
    with pytest.raises(ValueError, match='more than 256'):
        entropy.parse_jpeg(_with_table(key, (bits257, [i & 255 for i in range(257)])))


# ------------------------------------------------------------------- defects --

def test_defects_with_hostile_tables():
    from jds import entropy
    bad = hh.defective_files()
    assert set(bad) == {'size12', 'all_ones'}
    good, exp = hh.case('flat8', 'sparse_random', 24, 40, '4:2:0', seed=9)[:2]
    for kind, f in bad.items():
        entropy.parse_jpeg(f)           # the headers are in order
        for S in (64, 1024):
            with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x'):
                entropy.host_decode_jpeg(f, S)
        assert np.array_equal(entropy.host_decode_jpeg(good, 64)[0], exp)


# ------------------------------------------------------------- sanitizer run --

def test_hd_window_against_naive_walk_under_host_sanitizers(tmp_path):
    """tools/hd_window_check.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: hd_window against a naive byte walk at every data-byte position
    of seeded buffers, hd_run's positions over an 0xFF-dense scan."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'hd_window_check'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'hd_window_check.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stderr == '', r.stderr[-4000:]
    windows, symbols = int(r.stdout.split()[0]), int(r.stdout.split()[2])
    assert windows > 100000 and symbols > 5000
