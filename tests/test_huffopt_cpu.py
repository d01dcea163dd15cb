"""CPU-side checks of the optimised Huffman tables (no GPU): tests/huffopt_ref.py's
construction against libjpeg's (the DHTs of Pillow optimize=True files), the
properties every table must have, the named histograms that drive K.3 and the
32-bit fallback, the library's host core (jds_selftest_huffopt, the code
k_ent_opt_tables shares) against the reference, the reference files through two
independent decoders and libjpeg, and the stand-alone sanitizer program
(tools/huffopt_host_san.cpp)."""
import functools
import io
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import huffopt_ref as hr
import interleaved_ref as ir
from conftest import ROOT
from oracle import cpu_ref
from oracle import jpeg_entropy as je

CASES = hr.histogram_cases()


@pytest.fixture(scope='module', autouse=True)
def built():
    from jds import build
    build.build()


# ------------------------------------------------------------ against libjpeg --

def _pillow_file(h, w, ss, seed):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 3)) * 85 + np.linspace(0, 160, w)[None, :, None]).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=75, optimize=True, subsampling=ss)
    return b.getvalue()


@pytest.mark.parametrize('h,w,mode,ss', [(64, 64, '4:2:0', 2), (48, 80, '4:4:4', 0), (32, 64, '4:2:2', 1),
                                         (16, 16, '4:2:0', 2)])
def test_tables_equal_the_dhts_of_pillow_optimize(h, w, mode, ss):
    data = _pillow_file(h, w, ss, h + w)
    d = ir.decode(data)
    assert d['interleaved']
    hist = {k: np.zeros(256, np.int64) for k in hr.CLASSES}
    pred = [0, 0, 0]
    for c, y, x in ir.mcu_order(h, w, mode):     # libjpeg counts the interleaved scan
        zz = d['padded'][c][y, x][je.ZIGZAG]
        for cls, sym, _, _ in je.block_symbols(zz, pred[c]):
            hist[cls + ('1' if c else '0')][sym] += 1
        pred[c] = int(zz[0])
    ft = hr.file_tables(data)
    for k in hr.CLASSES:
        bits, vals, fell = hr.optimal_table(hist[k], hr.STD[k])
        assert not fell and (bits, vals) == ft[k], k


# ------------------------------------------------------------------ properties --

@pytest.mark.parametrize('name', sorted(CASES))
def test_table_properties(name):
    freq = CASES[name]
    bits, vals, fell = hr.optimal_table(freq)
    deep = hr.unconstrained_length(freq)
    if fell:
        assert deep > 32 and (bits, vals) == (list(je.AC_LUMA[0]), list(je.AC_LUMA[1]))
        return
    counted = [i for i in range(256) if freq[i]]
    assert sorted(vals) == counted                      # every counted symbol once, no other
    assert len(bits) == 16 and sum(bits) == len(vals)   # lengths <= 16
    codes = je.huffman_codes((bits, vals))
    assert all(code != (1 << length) - 1 for code, length in codes.values())   # no code is all ones
    kraft = sum(Fraction(b, 1 << (i + 1)) for i, b in enumerate(bits))
    longest = max((i + 1 for i, b in enumerate(bits) if b), default=0)
    assert kraft + Fraction(1, 1 << longest) <= 1 if longest else kraft == 0   # room for the reserved code
    if deep <= 16 and longest:
        # K.3 did not act: the code is a plain Huffman code, the reserved symbol on the one free code
        rest = 1 - kraft
        reserved = rest.denominator.bit_length() - 1
        assert rest == Fraction(1, 1 << reserved)
        assert hr.table_cost(freq, (bits, vals)) + reserved == hr.plain_huffman_cost(freq)


def test_named_histograms():
    f17, f18, f32, f33 = (hr.fibonacci(n) for n in (17, 18, 32, 33))
    assert f17.sum() == 6763 and hr.unconstrained_length(f17) == 17
    assert hr.optimal_table(f17)[0] == [1] * 14 + [0, 3]
    assert hr.unconstrained_length(f18) == 18
    assert hr.optimal_table(f18)[0] == [1] * 13 + [0, 2, 3]
    assert hr.unconstrained_length(f32) == 32 and not hr.optimal_table(f32)[2]
    assert f33.sum() == 14930350 and hr.unconstrained_length(f33) == 33 and hr.optimal_table(f33)[2]
    assert any(16 < hr.unconstrained_length(f) <= 32 for n, f in CASES.items() if n.startswith('random'))


# ------------------------------------------------------------------- host core --

@pytest.mark.parametrize('name', sorted(CASES))
def test_host_core_equals_the_reference(name):
    from jds import entropy
    assert entropy.optimal_table(CASES[name]) == hr.optimal_table(CASES[name])


def test_host_core_on_an_empty_histogram():
    from jds import entropy
    assert entropy.optimal_table(np.zeros(256)) == hr.optimal_table(np.zeros(256)) == ([0] * 16, [], False)


# ------------------------------------------------------------- reference files --

@functools.lru_cache(maxsize=None)
def codec_coeffs(kind, h, w, mode, q):
    rng = np.random.default_rng(q + h)
    if kind == 'noise':
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 255 // (h + w))], -1)
        img = np.clip(img + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, mode != '4:4:4', metrics=False)
    return np.asarray(ref['coeffs'], np.int16).reshape(-1), np.asarray(ref['qtable'], np.float64)


def _std_file(cf, h, w, mode, qt):
    ny, nc = hr.counts(h, w, mode)
    return je.encode_jfif(cf, h, w, mode, qt, ny, nc)[0]


@pytest.mark.parametrize('ri', [0, 64])
@pytest.mark.parametrize('h,w,mode', [(64, 96, '4:2:0'), (48, 80, '4:4:4'), (32, 64, '4:2:2')])
def test_reference_files_decode_to_their_coefficients(h, w, mode, ri):
    cf, qt = codec_coeffs('noise', h, w, mode, 50)
    data, bits, tabs = hr.encode_jfif_opt(cf, h, w, mode, qt, ri)
    d = ir.decode(data)                                  # reads the file's own DHTs
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in d['planar']]), cf)
    assert d['ri'] == ri and {('dc', 'ac')[k[0]] + str(k[1]): v for k, v in d['huff'].items()} == \
        {k: (t[0], t[1]) for k, t in tabs.items()}
    # oracle.jpeg_entropy.decode_jfif knows only the Annex K tables: it reads the file once the
    # frame's tables are put in their place
    if not ri:
        saved = je.DC_LUMA, je.AC_LUMA, je.DC_CHROMA, je.AC_CHROMA
        try:
            je.DC_LUMA, je.AC_LUMA, je.DC_CHROMA, je.AC_CHROMA = (tabs[k][:2] for k in hr.CLASSES)
            assert np.array_equal(je.decode_jfif(data)['coeffs'], cf)
        finally:
            je.DC_LUMA, je.AC_LUMA, je.DC_CHROMA, je.AC_CHROMA = saved
    Image = pytest.importorskip('PIL.Image')
    a = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    b = np.asarray(Image.open(io.BytesIO(_std_file(cf, h, w, mode, qt))).convert('RGB'))
    assert a.shape == (h, w, 3) and np.array_equal(a, b)


@pytest.mark.parametrize('q', [20, 50, 90])
@pytest.mark.parametrize('kind', ['noise', 'gradient'])
def test_reference_files_are_smaller_on_codec_frames(kind, q):
    h, w, mode = 64, 96, '4:2:0'
    cf, qt = codec_coeffs(kind, h, w, mode, q)
    assert len(hr.encode_jfif_opt(cf, h, w, mode, qt)[0]) < len(_std_file(cf, h, w, mode, qt))


def test_prescribed_histogram_builder():
    hist = hr.steep_ac_histogram([int(v) for v in hr.fibonacci(17)[:17]], 10)
    blk = hr.blocks_with_ac_histogram(169, hist)
    cf = np.concatenate([blk, np.zeros((2 * 169, 64), np.int16)])
    got = hr.histograms(cf, 104, 104, '4:4:4')['ac0']
    assert {s: int(c) for s, c in enumerate(got) if c} == hist
    assert hr.unconstrained_length(got) == 17            # K.3 runs on this frame's AC luma table


# ------------------------------------------------------------------- sanitizer --

def test_host_core_under_sanitizers(tmp_path):
    """tools/huffopt_host_san.cpp (its own main, no HIP, nothing loaded into Python) built with
    -fsanitize=address,undefined: the host core against a naive restatement."""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('clang++'), shutil.which('g++'))
                if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path / 'huffopt_host_san'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'jpeg-dsp-studio_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'huffopt_host_san.cpp'), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'ok' in r.stdout
