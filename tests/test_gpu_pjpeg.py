"""GPU checks of progressive files (csrc/jds_pjpeg_dec.hip: k_pjpeg_chains behind
jds_pjpeg_decode, jds_pjpeg_batch_to_rgb and jds_pjpeg_batch_transcode; DESIGN.md "Progressive
files").  The yardsticks: Pillow (libjpeg) wherever Pillow made the file -- its progressive and
baseline files of one array hold the same coefficients -- and tests/progressive_ref.py for the
scan scripts Pillow never writes.  Every comparison is an equality.  Small files, except the one
whose end-of-band run has to reach 32767."""
import numpy as np
import pytest

import interleaved_ref as il
import pjpeg_cases as pc
from test_jpeg_scale_cpu import draft_pixels
from test_pjpeg_cpu import build_pjpeg_san, run_pjpeg_san

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


# ------------------------------------------------------------ 1. Pillow's files --

@pytest.mark.parametrize('H,W,ss,rst,q', pc.PILLOW_PARAMS, ids=pc.PILLOW_IDS)
def test_gpu_pillow_progressive_files(H, W, ss, rst, q):
    """The transcode's twin of a restart file is Pillow's file of the same array without restart
    markers: the writer joins the intervals, as jpeg_transcode does."""
    from jds import codec, entropy
    arr, prog, base, kw = pc.pillow_pair(H, W, ss, rst, q)
    d = entropy.decode_pjpeg(prog)
    if ss == 'L':
        import gray_ref
        want = gray_ref.decode(base)['planar']
    else:
        want = il.decode(base)['planar']
    assert d['complete'] and d['status'] == 0 and np.array_equal(d['coeffs'], want)
    assert np.array_equal(codec.pjpeg_to_rgb(prog, render='libjpeg'), pc.pillow_rgb(prog))
    for dn in (2, 4, 8):
        got = codec.pjpeg_to_rgb(prog, render='libjpeg', scale_denom=dn)
        exp = draft_pixels(prog, dn) if H >= dn and W >= dn else codec.jpeg_to_rgb(base, render='libjpeg', scale_denom=dn)
        assert got.shape == (-(-H // dn), -(-W // dn), 3) and np.array_equal(got, exp), dn
    assert np.array_equal(codec.pjpeg_to_rgb(prog, render='reference'), codec.jpeg_to_rgb(base))
    plain = {k: v for k, v in kw if k != 'restart_marker_rows'}
    assert codec.pjpeg_transcode(prog, optimize=True) == pc.save(arr, optimize=True, **plain)
    assert codec.pjpeg_transcode(prog, optimize=False) == pc.save(arr, **plain)


def test_gpu_pjpeg_to_rgb_on_a_device_tensor_and_with_info():
    import torch
    from jds import codec
    arr, prog, base, _ = pc.pillow_pair(37, 53, 1, 0, 75)
    out = torch.full((19, 27, 3), 0x5A, dtype=torch.uint8, device='cuda')
    got, info = codec.pjpeg_to_rgb(prog, out=out, scale_denom=2, with_info=True)
    assert got is out and (info['scale_denom'], info['out_H'], info['out_W'], info['route']) == (2, 19, 27, 'chains')
    assert np.array_equal(out.cpu().numpy(), draft_pixels(prog, 2))
    assert np.array_equal(info['coeffs'], pc.reference(prog)) and len(info['scans']) == 10
    with pytest.raises(ValueError, match=r'\(19, 27, 3\)'):
        codec.pjpeg_to_rgb(prog, out=torch.empty((37, 53, 3), dtype=torch.uint8, device='cuda'), scale_denom=2)
    with pytest.raises(ValueError, match='not progressive'):
        codec.pjpeg_to_rgb(base)
    with pytest.raises(ValueError, match='progressive'):        # and the existing call is untouched
        codec.jpeg_to_rgb(prog)


# ----------------------------------------- 2. scan scripts Pillow never writes --

@pytest.mark.parametrize('H,W,mode,name', pc.SCRIPT_PARAMS, ids=pc.SCRIPT_IDS)
def test_gpu_scripted_files(H, W, mode, name):
    from jds import codec, entropy
    f, padded, complete = pc.script_file(H, W, mode, name)
    ref = pc.reference(f)
    d = entropy.decode_pjpeg(f)
    assert d['status'] == 0 and d['complete'] == complete and np.array_equal(d['coeffs'], ref)
    # the transcode is the baseline file of the same coefficients, whatever the script
    for optimize in (True, False):
        t = codec.pjpeg_transcode(f, optimize=optimize)
        assert not codec.is_progressive(t) and np.array_equal(il.decode(t)['planar'], ref)
    if not complete:
        with pytest.raises(ValueError, match='incomplete progression'):
            codec.pjpeg_to_rgb(f)
        return
    got = codec.pjpeg_to_rgb(f, render='libjpeg')
    assert np.array_equal(got, codec.jpeg_to_rgb(t, render='libjpeg'))
    if name != 'full_amplitude':     # (pixels far outside [0, 255]: libjpeg's C and SIMD inverses differ there)
        assert np.array_equal(got, pc.pillow_rgb(f))


def test_gpu_eobrun_32767():
    """33,124 blocks whose AC scan is one run of 32767, one of 356 and a coefficient: the run is
    emitted at its limit and counted again."""
    from jds import entropy
    f, planar = pc.eobrun_file()
    o = entropy.parse_pjpeg(f)['scans'][1]['ac_dht'][0]
    assert 0xE0 in f[o + 17:o + 17 + sum(f[o + 1:o + 17])]           # (the AC scan's table has EOB14)
    d = entropy.decode_pjpeg(f)
    assert d['status'] == 0 and np.array_equal(d['coeffs'], planar)


# ------------------------------------------------------------ 3. hostile scans --

GUARD = 64


def _decode_between_guards(f):
    import torch
    from jds import entropy
    need = entropy.parse_pjpeg(f)['coeffs_needed']
    buf = torch.full((need + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device='cuda')
    torch.cuda.synchronize()                  # (a raw pointer: the call does not wait for the fill)
    d = entropy.decode_pjpeg_dev(f, buf.data_ptr() + 2 * GUARD, need)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0x5A5A).all() and (h[-GUARD:] == 0x5A5A).all()
    return d, h[GUARD:-GUARD]


def test_gpu_hostile_scans(tmp_path):
    """Each hostile file first through the sanitizer program (parser and host model of the same
    core), then on the device: a status, no exception from the device, the guard words around the
    coefficients intact; in a batch the neighbours' outputs are what they are alone."""
    from jds import codec, entropy
    hostile = pc.hostile_files()
    san = run_pjpeg_san(build_pjpeg_san(tmp_path), tmp_path, hostile)
    assert len(san) == len(hostile) and all(rc == 0 and st != 0 for rc, st in san.values()), san
    good = pc.script_file(24, 40, '4:2:0', 'bands')[0]
    d, cf = _decode_between_guards(good)
    assert d['status'] == 0 and np.array_equal(cf, pc.reference(good))
    for name, f in hostile.items():
        d, _ = _decode_between_guards(f)
        assert d['status'] != 0 and d['status'] == san[name][1], name
        with pytest.raises(ValueError, match='defective scan data'):
            entropy.decode_pjpeg(f)
        with pytest.raises(ValueError, match='defective scan data'):
            codec.pjpeg_to_rgb(f)
        with pytest.raises(ValueError, match='defective scan data'):
            codec.pjpeg_transcode(f)
    # the context is still good, and neighbours in a batch do not notice
    a, b = pc.pillow_pair(40, 56, 2, 0, 75)[1], pc.pillow_pair(17, 33, 0, 0, 75)[1]
    files = [a] + [x for f in hostile.values() for x in (f, b, a)]
    imgs, info = codec.pjpeg_batch_to_rgb(files, out=None, errors='return', with_info=True)
    outs, items = codec.pjpeg_batch_transcode(files, errors='items')
    ia, ib, ta, tb = codec.pjpeg_to_rgb(a), codec.pjpeg_to_rgb(b), codec.pjpeg_transcode(a), codec.pjpeg_transcode(b)
    for i, f in enumerate(files):
        if f is a or f is b:
            assert np.array_equal(imgs[i], ia if f is a else ib) and outs[i] == (ta if f is a else tb), i
        else:
            assert imgs[i] is None and outs[i] is None
            assert info['items'][i]['rc'] == 0 and info['items'][i]['status'] != 0 and items[i]['status'] != 0


# ------------------------------------------------------------- 4. mixed batch --

def _mixed():
    prog = [pc.pillow_pair(h, w, ss, r, 75)[1] for h, w, ss, r in pc.PILLOW_SIZES if (h, w) not in ((200, 264), (264, 200))]
    prog.append(pc.script_file(24, 40, '4:2:0', 'bands')[0])
    assert len(prog) == 8
    return prog + [pc.pillow_pair(40, 56, 2, 0, 75)[2], pc.hostile_files()['ones_in_scan_1']]


def test_gpu_mixed_batch_to_rgb():
    from jds import codec
    files = _mixed()
    imgs, info = codec.pjpeg_batch_to_rgb(files, out=None, errors='return', with_info=True)
    dev = codec.pjpeg_batch_to_rgb(files, errors='return')                     # out='device'
    off = 0
    for i, f in enumerate(files):
        it = info['items'][i]
        if i < 8:
            assert it['rc'] == 0 and it['status'] == 0 and it['rgb_off'] == off and off % 256 == 0
            off += -(-it['H'] * it['W'] * 3 // 256) * 256
            assert np.array_equal(imgs[i], codec.pjpeg_to_rgb(f)) and np.array_equal(imgs[i], pc.pillow_rgb(f))
            assert np.array_equal(dev[i].cpu().numpy(), imgs[i])
        else:
            assert imgs[i] is None and dev[i] is None
    assert info['items'][8]['rc'] != 0 and info['items'][8]['rgb_off'] == -1
    assert info['items'][9]['rc'] == 0 and info['items'][9]['status'] != 0 and info['items'][9]['rgb_off'] == off
    assert info['rgb_bytes'] == off + -(-24 * 40 * 3 // 256) * 256
    with pytest.raises(ValueError, match=r'file 8: not progressive \(SOF0\)'):
        codec.pjpeg_batch_to_rgb(files, out=None)
    # denominators per file, as the namesake takes them
    dens = [1, 2, 4, 8, 2, 4, 8, 1, 1, 1]
    scaled = codec.pjpeg_batch_to_rgb(files, out=None, errors='return', scale_denom=dens)
    for i in range(8):
        assert np.array_equal(scaled[i], codec.pjpeg_to_rgb(files[i], scale_denom=dens[i])), i
    assert codec.pjpeg_batch_to_rgb([], out=None) == []


def test_gpu_mixed_batch_transcode():
    from jds import codec
    files = _mixed()
    outs, items = codec.pjpeg_batch_transcode(files, errors='items')
    dev, ditems = codec.pjpeg_batch_transcode(files, errors='items', out='device')
    off = 0
    for i, f in enumerate(files[:8]):
        assert items[i]['rc'] == 0 and items[i]['status'] == 0 and items[i]['out_off'] == off and off % 256 == 0
        off += -(-items[i]['out_len'] // 256) * 256
        assert outs[i] == codec.pjpeg_transcode(f) and bytes(dev[i].cpu().numpy()) == outs[i]
    assert ditems == items
    assert outs[8] is None and items[8]['rc'] != 0 and items[8]['out_off'] == -1
    assert outs[9] is None and items[9]['rc'] == 0 and items[9]['status'] != 0
    with pytest.raises(ValueError, match=r'file 8: not progressive \(SOF0\)'):
        codec.pjpeg_batch_transcode(files)
    # the device output feeds the existing batch call, which renders Pillow's pixels of the originals
    back = codec.jpeg_batch_to_rgb([t.cpu().numpy() for t in dev[:8]], render='libjpeg')
    for i in range(8):
        assert np.array_equal(back[i], pc.pillow_rgb(files[i])), i


# ------------------------------------------- 5. both front ends on one context --

def test_gpu_both_front_ends_share_one_contexts_batch_buffers():
    """The baseline and the progressive batch calls share one driver and one pair of staging and
    device buffers per context: batch sizes go up and then down on one caller-owned Context, so
    each front end runs in buffers the other grew, with stale contents beyond its own upload.
    Every image is Pillow's decode of the same file."""
    from jds import _abi, codec
    small = [pc.pillow_pair(9, 9, 2, 0, 75), pc.pillow_pair(24, 40, 'L', 0, 75), pc.pillow_pair(40, 56, 2, 0, 75)]
    prog, base = [p[1] for p in small], [p[2] for p in small]
    big = [pc.pillow_pair(200, 264, 2, 0, 75)[2], pc.pillow_pair(264, 200, 0, 0, 75)[2]]
    one = pc.pillow_pair(1, 1, 0, 0, 75)[1]
    ctx = _abi.Context(0)
    try:
        imgs = codec.pjpeg_batch_to_rgb(prog, out=None, ctx=ctx)
        for f, im in zip(prog, imgs):
            assert np.array_equal(im, pc.pillow_rgb(f))
        imgs = codec.jpeg_batch_to_rgb(big, render='libjpeg', ctx=ctx)
        for f, im in zip(big, imgs):
            assert np.array_equal(im, pc.pillow_rgb(f))
        dev = codec.pjpeg_batch_transcode(prog, out='device', ctx=ctx)
        back = [t.cpu().numpy() for t in dev]
        imgs = codec.jpeg_batch_to_rgb(back, render='libjpeg', ctx=ctx)
        for f, t, im in zip(prog, back, imgs):
            assert not codec.is_progressive(t) and np.array_equal(im, pc.pillow_rgb(bytes(t)))
            assert np.array_equal(im, pc.pillow_rgb(f))
        imgs = codec.pjpeg_batch_to_rgb([one], ctx=ctx)                       # out='device'
        assert np.array_equal(imgs[0].cpu().numpy(), pc.pillow_rgb(one))
        dens = [1, 2, 4]
        imgs = codec.jpeg_batch_to_rgb(base, render='libjpeg', scale_denom=dens, ctx=ctx)
        for f, dn, im in zip(base, dens, imgs):
            assert np.array_equal(im, pc.pillow_rgb(f) if dn == 1 else draft_pixels(f, dn)), dn
    finally:
        ctx.close()
