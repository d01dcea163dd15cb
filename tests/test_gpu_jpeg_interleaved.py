"""GPU checks of the interleaved-scan decoder (jds_decode_jpeg; the interleaved
instantiations of k_dec_sync / k_dec_write / k_dec_rst and k_dec_dc_mcu):
bit-equality with the reference decoder (tests/interleaved_ref.py) on the
Pillow-written fixtures and on writer-made files that span workgroups, the
sequential all-zero regime and its wrong-slot variant, both restart routes,
defective scan data, and decompress_jpeg's two routes."""
import io

import numpy as np
import pytest

import interleaved_ref as ir
import restart_ref as rr
from oracle import cpu_ref
from oracle import jpeg_entropy as je
from test_jpeg_interleaved_cpu import MANIFEST, NAMES, Q50, QC, fixture, oracle_image, written, zero_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


@pytest.mark.parametrize('name', NAMES)
def test_gpu_decodes_fixture(name):
    from jds import entropy
    data, exp = fixture(name)
    d = entropy.decode_jpeg(data)
    assert d['coeffs'].dtype == np.int16 and np.array_equal(d['coeffs'], exp), f"rounds {d['rounds']}"
    assert [list(g) for g in d['grids']] == MANIFEST['files'][name]['grids']
    assert (d['rounds'] == 0) == bool(MANIFEST['files'][name]['restart_interval'])


@pytest.mark.parametrize('mode', ['4:2:0', '4:2:2', '4:4:4'])
def test_gpu_scan_spans_workgroups(mode):
    """Dense noise blocks: the one scan is longer than two workgroups' subsequences."""
    from jds import entropy
    S, G = entropy.decode_info()
    h, w = 185, 199
    rng = np.random.default_rng(11)
    padded = ir.random_padded(rng, h, w, mode, amp=300, density=0.9)
    data = ir.write(padded, h, w, mode, {0: Q50, 1: QC})
    exp = ir.crop(padded, ir.geometry(h, w, mode)[1])
    sc = entropy.parse_jpeg(data)['scans'][0]
    ngroups = -(-8 * sc['length'] // (S * G))
    assert ngroups >= 3, (sc['length'], S, G)
    d = entropy.decode_jpeg(data)
    assert np.array_equal(d['coeffs'], exp)
    assert 1 <= d['rounds'] <= ngroups


@pytest.mark.parametrize('variant', [False, True])
def test_gpu_zero_coefficient_file(variant):
    """All coefficients zero: 32-bit MCUs, nothing to synchronise on.  The variant (one AC
    coefficient per Cb block) breaks the MCU length's divisibility, so guesses land in wrong
    slots (tests/test_jpeg_interleaved_cpu.py shows the rounds on the host model)."""
    from jds import entropy
    data, exp = zero_file(variant, 96, 80)
    d = entropy.decode_jpeg(data)
    assert np.array_equal(d['coeffs'], exp) and d['rounds'] >= 1


@pytest.mark.parametrize('h,w,mode,ri', [(41, 66, '4:2:0', 2), (33, 35, '4:2:2', 4), (160, 160, '4:2:0', 64), (150, 160, '4:2:0', 64),
                                        (41, 50, '4:2:0', 1)])
def test_gpu_restart_routes(h, w, mode, ri):
    """Lane route (Ri * blocks per MCU <= lane_max_blocks) and descriptor route (64 MCUs = 384
    blocks: intervals of 64 and 36 MCUs); a last short interval; padding blocks in all but
    160x160, which is whole MCUs."""
    from jds import entropy
    data, padded, exp = written(h, w, mode, 5 * h + ri, ri=ri)
    d = entropy.parse_jpeg(data)
    nmcu, bpm = d['mcu']['rows'] * d['mcu']['cols'], d['mcu']['blocks']
    assert ri == 1 or nmcu % ri
    assert (h, w) == (160, 160) or sum(p.shape[0] * p.shape[1] for p in padded) * 64 > exp.size
    lane = ri * bpm <= entropy.restart_info()[1]
    assert lane == (ri != 64)
    out = entropy.decode_jpeg(data)
    assert np.array_equal(out['coeffs'], exp)
    assert (out['rounds'] == 0) == lane


def test_gpu_dc_chain_through_padding():
    from jds import entropy
    for ri in (0, 1):
        data, padded, exp = written(17, 23, '4:2:0', 77 + ri, pad_dc=1000, ri=ri)
        assert np.array_equal(entropy.decode_jpeg(data)['coeffs'], exp)


def _rejected_by_reference(data):
    try:
        ir.decode(data)
    except (AssertionError, IndexError, KeyError):
        return True
    return False


def _defects(data):
    """{kind: file}: the scan cut in half; one bit flipped in its middle; the last RSTm removed.
    A flipped magnitude bit leaves a well-formed file with another coefficient, which no decoder
    can tell from the original, so the bit is the first one from the middle of the scan on whose
    flip the reference decoder (tests/interleaved_ref.py) fails; bytes that are or neighbour an
    0xFF are left alone, so that no marker or stuffing appears or vanishes."""
    from jds import entropy
    sc = entropy.parse_jpeg(data)['scans'][0]
    a, n = sc['offset'], sc['length']
    out = {'truncated': data[:a + n // 2] + data[a + n:]}
    for bit in range(8 * (a + n // 2), 8 * (a + n - 2)):
        i, m = bit >> 3, 0x80 >> (bit & 7)
        if 0xFF in data[i - 1:i + 2] or data[i] ^ m == 0xFF:
            continue
        f = data[:i] + bytes([data[i] ^ m]) + data[i + 1:]
        if _rejected_by_reference(f):
            out['flipped'] = f
            break
    pos = [i for i in range(a, a + n - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    if pos:
        out['rst_removed'] = data[:pos[-1]] + data[pos[-1] + 2:]
    return out


DEFECT_NAMES = ['p24x40_420', 'p33x35_422', 'p9x9_444', 'p40x72_420_rst2', 'p48x48_420_opt_rstrow',
                'p31x45_420_q95_opt']


@pytest.mark.parametrize('name', DEFECT_NAMES)
def test_gpu_defective_files_raise(name):
    """Ordinary bounded decodes of bad data: each is a ValueError naming the defect (a removed
    RSTm is caught by the parser's marker count), and the context decodes the next file."""
    from jds import entropy
    data, exp = fixture(name)
    bad = _defects(data)
    assert ('rst_removed' in bad) == bool(MANIFEST['files'][name]['restart_interval']) and 'flipped' in bad
    assert all(_rejected_by_reference(f) for f in bad.values())
    for kind, f in bad.items():
        with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x|restart markers where DRI'):
            entropy.decode_jpeg(f)
    assert np.array_equal(entropy.decode_jpeg(data)['coeffs'], exp)


def test_gpu_decompress_plan_route():
    """One table, reference grid: the plan's inverse, byte-equal to decompress_jfif of the
    library's own file of the same coefficients and to the staged route forced on the file."""
    from jds import codec, entropy
    h, w, mode, q = 48, 80, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 3)
    raw = codec.compress_reconstruct_raw(img, q, Q50, mode, True, maps=False)
    own, _ = entropy.encode_jfif(raw['coeffs'], h, w, mode, Q50)
    _, grids, _ = ir.geometry(h, w, mode)
    blocks, b0, padded = raw['coeffs'].reshape(-1, 64), 0, []
    for (gr, gc), (pr, pc) in zip(grids, ir.padded_shapes(h, w, mode)):
        p = np.zeros((pr, pc, 64), np.int64)
        p[:gr, :gc] = blocks[b0:b0 + gr * gc].reshape(gr, gc, 64)
        b0 += gr * gc
        padded.append(p)
    data = ir.write(padded, h, w, mode, {0: Q50}, (0, 0, 0))
    a, info = codec.decompress_jpeg(data, with_info=True)
    assert info['route'] == 'plan' and np.array_equal(info['coeffs'], raw['coeffs'])
    assert np.array_equal(a, codec.decompress_jfif(own))
    assert np.array_equal(a, raw['reconstructed'])
    b, info = codec.decompress_jpeg(data, with_info=True, staged=True)
    assert info['route'] == 'staged' and np.array_equal(a, b)


@pytest.mark.parametrize('name', NAMES)
def test_gpu_decompress_staged_route(name):
    from jds import codec
    data, exp = fixture(name)
    img, info = codec.decompress_jpeg(data, with_info=True)
    assert info['route'] == 'staged'
    ref = oracle_image(exp, info['H'], info['W'], info['mode'], info['qtables'], info['grids'])
    assert img.dtype == np.uint8 and np.array_equal(img, ref)


def test_gpu_live_pillow_round_trip():
    Image = pytest.importorskip('PIL.Image')
    from jds import codec, entropy
    for seed, (h, w), sub in ((1, (50, 70), 2), (2, (64, 48), 0)):
        rgb = cpu_ref.random_image(h, w, seed)
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, 'JPEG', quality=75, subsampling=sub)
        data = buf.getvalue()
        assert np.array_equal(entropy.decode_jpeg(data)['coeffs'], ir.decode(data)['planar'])
        img = codec.decompress_jpeg(data)
        diff = np.abs(img.astype(int) - np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).astype(int))
        # reported, not asserted: the two inverses differ by design (IDCT arithmetic, chroma upsampling)
        print(f'{h}x{w} subsampling {sub}: vs Pillow max {diff.max()} mean {diff.mean():.3f}')


def test_gpu_existing_paths_unchanged():
    from jds import codec, entropy
    h, w, mode = 40, 56, '4:2:2'
    ny, nc = rr.counts(h, w, mode)
    cf = np.random.default_rng(4).integers(-30, 31, (ny + 2 * nc) * 64).astype(np.int16)
    for data in (je.encode_jfif(cf, h, w, mode, Q50, ny, nc)[0], rr.encode_jfif_rst(cf, h, w, mode, Q50, 7)[0]):
        assert np.array_equal(entropy.decode_jfif(data)['coeffs'], cf)
        d = entropy.decode_jpeg(data)       # the same file through the new entry point
        assert np.array_equal(d['coeffs'], cf) and not d['interleaved']
        a = codec.decompress_jfif(data)
        assert np.array_equal(a, codec.decompress_jpeg(data)) and np.array_equal(a, codec.decompress_jpeg(data, staged=True))
    with pytest.raises(ValueError, match='two quantisation tables|interleaved scan'):
        entropy.decode_jfif(fixture('p24x40_420')[0])


def test_gpu_one_context_alternates_scan_forms():
    """The single-file calls serve both scan forms over the same context buffers: lanes,
    one descriptor, and descriptors per interval, interleaved and not, in turn on one
    context.  A stale interval table, MCU record or DC staging array of the previous file
    would show; the first file decodes the same again at the end."""
    import ctypes as C
    from jds import _abi, entropy
    lane_max = entropy.restart_info()[1]
    rstrow, small, rst2 = (fixture(n)[0] for n in ('p48x48_420_opt_rstrow', 'p9x9_444', 'p40x72_420_rst2'))
    own = entropy.encode_jfif(fixture('p9x9_444')[1], 16, 16, '4:4:4', Q50)[0]   # (2 x 2 blocks per component, as 9x9)
    ny, nc = rr.counts(40, 56, '4:2:0')
    blocks = fixture('p40x72_420_rst2')[1].reshape(-1, 64)[:ny + 2 * nc]
    plain5 = rr.encode_jfif_rst(blocks.reshape(-1), 40, 56, '4:2:0', Q50, 5)[0]
    il = [entropy.parse_jpeg(d)['interleaved'] for d in (rstrow, small, rst2, plain5)]
    assert il == [True, True, True, False] and 5 <= lane_max
    order = [(rstrow, False), (own, True), (small, False), (rst2, False), (plain5, False), (rstrow, False)]
    got = []
    with _abi.lease(0) as ctx:
        for data, jfif in order:
            a, p, n = entropy._bytes_arg(data)
            info = _abi.JfifInfo() if jfif else _abi.JpegInfo()
            _abi.check((_abi.lib().jds_jfif_parse if jfif else _abi.lib().jds_jpeg_parse)(p, n, C.byref(info)))
            cf = np.full(int(info.coeffs_needed), 0x5555, np.int16)
            call = _abi.lib().jds_decode_jfif if jfif else _abi.lib().jds_decode_jpeg
            _abi.check(call(ctx.handle, p, n, cf.ctypes.data, cf.size, C.byref(info)))
            got.append(cf)
    for (data, jfif), cf in zip(order, got):
        exp = (entropy.host_decode_jfif if jfif else entropy.host_decode_jpeg)(data)[0]
        assert np.array_equal(cf, exp)
    assert np.array_equal(got[0], got[-1])


def test_gpu_one_context_single_and_batch_calls_in_turn():
    """A single-file call is the batch driver's batch of one, so on one context the single calls
    and the batch calls take turns on the same upload buffer, pinned staging, scratch and DC
    staging array: decode, batch render, decode of the other scan form by descriptors per
    interval, render into a device tensor, batch transcode, transcode, transform, and the first
    decode again.  Every result is the host model's; the first and the last are equal."""
    import ctypes as C
    import torch
    from jds import _abi, codec, entropy
    lib, lane_max = _abi.lib(), entropy.restart_info()[1]
    rstrow, small, rst2 = (fixture(n)[0] for n in ('p48x48_420_opt_rstrow', 'p9x9_444', 'p40x72_420_rst2'))
    ny, nc = rr.counts(40, 56, '4:2:0')
    plain5 = rr.encode_jfif_rst(fixture('p40x72_420_rst2')[1][:(ny + 2 * nc) * 64], 40, 56, '4:2:0', Q50, 5)[0]
    ny, nc = rr.counts(96, 104, '4:2:0')      # 156 luma blocks: intervals of 130 and 26 blocks, each a descriptor
    wide = rr.encode_jfif_rst(np.random.default_rng(96).integers(-9, 10, (ny + 2 * nc) * 64).astype(np.int16), 96, 104,
                              '4:2:0', Q50, lane_max + 2)[0]
    d = entropy.parse_jpeg(rstrow)
    assert d['interleaved'] and d['scans'][0]['restart_interval'] * d['mcu']['blocks'] <= lane_max
    assert not entropy.parse_jpeg(wide)['interleaved'] and ny > lane_max + 2 and (d['H'], d['W']) == (48, 48)

    def host_image(data):
        p = entropy.parse_jpeg(data)
        return codec.host_jpeg_render(entropy.host_decode_jpeg(data)[0], p['H'], p['W'], p['mode'], p['qtables'],
                                      p['grids'], render='reference')

    def decode(ctx, data):
        a, p, n = entropy._bytes_arg(data)
        info = _abi.JpegInfo()
        _abi.check(lib.jds_jpeg_parse(p, n, C.byref(info)))
        cf = np.full(int(info.coeffs_needed), 0x5555, np.int16)
        _abi.check(lib.jds_decode_jpeg(ctx.handle, p, n, cf.ctypes.data, cf.size, C.byref(info)))
        return cf

    def rewritten(ctx, data, xf=None):
        a, p, n = entropy._bytes_arg(data)
        info = _abi.JpegInfo()
        if xf is None:
            return entropy._grown(lambda o, cap, m: lib.jds_jpeg_transcode(ctx.handle, p, n, 1, o.ctypes.data, cap,
                                                                           C.byref(m), C.byref(info)), 2 * n)
        return entropy._grown(lambda o, cap, m: lib.jds_jpeg_transform(ctx.handle, p, n, _abi.xf_code(xf), 1, o.ctypes.data,
                                                                       cap, C.byref(m), C.byref(info)), 2 * n)

    with _abi.lease(0) as ctx:
        first = decode(ctx, rstrow)
        imgs = codec.jpeg_batch_to_rgb([small, plain5, rst2], ctx=ctx)
        cf_wide = decode(ctx, wide)
        a, p, n = entropy._bytes_arg(rst2)
        info = _abi.JpegInfo()
        dev = torch.full((40, 72, 3), 0xA5, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        _abi.check(lib.jds_jpeg_to_rgb(ctx.handle, p, n, C.c_void_p(int(dev.data_ptr())), dev.numel(), 1, None, C.byref(info)))
        outs = codec.jpeg_batch_transcode([rstrow, plain5], ctx=ctx)
        one = rewritten(ctx, small)
        turned = rewritten(ctx, rstrow, 'rot90')
        last = decode(ctx, rstrow)
    assert np.array_equal(first, entropy.host_decode_jpeg(rstrow)[0]) and np.array_equal(first, last)
    for img, data in zip(imgs, (small, plain5, rst2)):
        assert np.array_equal(img, host_image(data))
    assert np.array_equal(cf_wide, entropy.host_decode_jpeg(wide)[0])
    assert np.array_equal(dev.cpu().numpy(), host_image(rst2))
    assert outs == [entropy.host_transcode_jpeg(f) for f in (rstrow, plain5)]
    assert one == entropy.host_transcode_jpeg(small)
    assert turned == entropy.host_transform_jpeg(rstrow, 'rot90')


def test_gpu_own_profile_files_through_both_decode_calls():
    """jds_decode_jfif runs on the general info like jds_decode_jpeg: a file with its scans in
    the order Cr, Y, Cb (the component-to-plane mapping) and one with restart intervals give,
    on one context, the host model's coefficients, status 0 and the same rounds through both
    calls; decompress_jfif and decompress_jpeg return the same bytes."""
    import ctypes as C
    from jds import _abi, codec, entropy
    from test_entropy_decode_cpu import codec_file
    data, _, _ = codec_file(33, 47, '4:4:4', 50)
    sos = data.index(b'\xff\xda')
    parts = [data[s['offset'] - 10:s['offset'] + s['length']] for s in entropy.parse_jfif(data)['scans']]
    shuffled = data[:sos] + parts[2] + parts[0] + parts[1] + b'\xff\xd9'
    assert [s['component'] for s in entropy.parse_jfif(shuffled)['scans']] == [3, 1, 2]
    ny, nc = rr.counts(40, 56, '4:2:0')
    cf = np.random.default_rng(4056).integers(-20, 21, (ny + 2 * nc) * 64).astype(np.int16)
    rst = rr.encode_jfif_rst(cf, 40, 56, '4:2:0', Q50, 7)[0]
    assert np.array_equal(entropy.host_decode_jfif(rst)[0], cf)
    with _abi.lease(0) as ctx:
        for f in (shuffled, rst):
            exp = entropy.host_decode_jfif(f)[0]
            a, p, n = entropy._bytes_arg(f)
            fi, ji = _abi.JfifInfo(), _abi.JpegInfo()
            got_f, got_j = np.empty(exp.size, np.int16), np.empty(exp.size, np.int16)
            _abi.check(_abi.lib().jds_decode_jfif(ctx.handle, p, n, got_f.ctypes.data, got_f.size, C.byref(fi)))
            _abi.check(_abi.lib().jds_decode_jpeg(ctx.handle, p, n, got_j.ctypes.data, got_j.size, C.byref(ji)))
            assert np.array_equal(got_f, exp) and np.array_equal(got_j, exp)
            assert fi.status == 0 and ji.status == 0 and fi.rounds == ji.rounds
            assert int(fi.coeffs_needed) == int(ji.coeffs_needed) == exp.size
    for f in (shuffled, rst):
        assert np.array_equal(codec.decompress_jfif(f), codec.decompress_jpeg(f))
