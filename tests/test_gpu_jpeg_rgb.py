"""GPU checks of the fused inverse for foreign JPEGs (jds_jpeg_to_rgb, jds_jpeg_inverse_dev;
k_jpeg_inv): byte equality with the definition of the staged inverse
(test_jpeg_interleaved_cpu.oracle_image) on the Pillow-written fixtures and on writer-made
files at tile edges, equality with the plan route and with decompress_jfif where those apply,
both scan forms, output left on the device (with guard bytes around it), defective scans, and
with_info."""
import numpy as np
import pytest

import interleaved_ref as ir
import restart_ref as rr
from oracle import cpu_ref
from oracle import jpeg_entropy as je
from test_jpeg_interleaved_cpu import NAMES, Q50, QC, fixture, oracle_image, written

pytestmark = pytest.mark.gpu

Q2 = np.clip(QC + 7, 1, 255)
MODES = ['4:2:0', '4:2:2', '4:4:4']


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def _sizes():
    from jds import build, codec
    build.build()
    th, tw = codec.jpeg_inverse_info()
    return [(1, 1), (1, 17), (2, 3), (7, 9), (15, 17), (th - 1, tw + 1), (th + 1, 2 * tw - 1), (2 * th + 1, tw + 1),
            (185, 199)]


def three_table_file(h, w, mode, seed):
    """A writer-made file with three distinct tables and coefficients that saturate both ends."""
    rng = np.random.default_rng(seed)
    padded = ir.random_padded(rng, h, w, mode, amp=300, density=0.9)
    grids = ir.geometry(h, w, mode)[1]
    data = ir.write(padded, h, w, mode, {0: Q50, 1: QC, 2: Q2}, tq=(0, 1, 2))
    return data, ir.crop(padded, grids), np.stack([Q50, QC, Q2]), grids


@pytest.mark.parametrize('name', NAMES)
def test_gpu_fixture_to_rgb(name):
    from jds import codec
    data, exp = fixture(name)
    d = ir.decode(data)
    img = codec.jpeg_to_rgb(data)
    assert img.dtype == np.uint8 and img.shape == (d['H'], d['W'], 3)
    assert np.array_equal(img, oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids']))
    assert np.array_equal(img, codec.decompress_jpeg(data, staged=True))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size', range(9))
def test_gpu_tile_edges(size, mode):
    """Partial tiles, one pixel past a tile in either direction, the halo between tiles, taps
    that are not 2x (odd sizes), the crop of the T.81 planes."""
    from jds import codec
    h, w = _sizes()[size]
    data, cf, qt, grids = three_table_file(h, w, mode, 100 * size + len(mode) + h)
    img = codec.jpeg_to_rgb(data)
    ref = oracle_image(cf, h, w, mode, qt, grids)
    assert np.array_equal(img, ref), (h, w, np.argwhere(img != ref)[:4])


def test_gpu_plan_eligible_file():
    """One table, the reference's grids: the fused inverse equals the plan's inverse, the
    library's own file through decompress_jfif, and compress_reconstruct_raw's reconstruction."""
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
    a = codec.jpeg_to_rgb(data)
    b, info = codec.decompress_jpeg(data, with_info=True)
    assert info['route'] == 'plan' and np.array_equal(a, b)
    assert np.array_equal(a, codec.decompress_jfif(own))
    assert np.array_equal(a, raw['reconstructed'])


def test_gpu_both_scan_forms():
    from jds import codec
    h, w, mode = 40, 56, '4:2:2'
    ny, nc = rr.counts(h, w, mode)
    cf = np.random.default_rng(4).integers(-30, 31, (ny + 2 * nc) * 64).astype(np.int16)
    for data in (je.encode_jfif(cf, h, w, mode, Q50, ny, nc)[0], rr.encode_jfif_rst(cf, h, w, mode, Q50, 7)[0]):
        img, info = codec.jpeg_to_rgb(data, with_info=True)
        assert not info['interleaved'] and np.array_equal(info['coeffs'], cf)
        assert np.array_equal(img, codec.decompress_jfif(data))


def test_gpu_output_stays_on_the_device():
    import torch
    from jds import codec
    data, exp = fixture('p31x45_420_q95_opt')
    host = codec.jpeg_to_rgb(data)
    h, w = host.shape[:2]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda')
    got = codec.jpeg_to_rgb(data, out=out)
    assert got is out
    assert np.array_equal(out.cpu().numpy(), host)
    with pytest.raises(ValueError, match='out must be'):
        codec.jpeg_to_rgb(data, out=torch.empty((h, w + 1, 3), dtype=torch.uint8, device='cuda'))


@pytest.mark.parametrize('lead', [64, 67])
def test_gpu_inverse_dev_writes_only_the_image(lead):
    """jpeg_inverse_dev on torch tensors and torch's stream; the image lies between guard bytes
    (0xA5) that the kernel's ordinary stores leave alone.  lead = 67 puts the image at an odd
    address: the byte-store path."""
    import torch
    from jds import codec, entropy
    th, tw = codec.jpeg_inverse_info()
    h, w, mode = th + 3, tw + 5, '4:2:0'
    data, cf, qt, grids = three_table_file(h, w, mode, 9)
    d = entropy.decode_jpeg(data)
    assert np.array_equal(d['coeffs'], cf)
    n = h * w * 3
    coeffs = torch.from_numpy(d['coeffs']).cuda()
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    codec.jpeg_inverse_dev(d, coeffs.data_ptr(), buf.data_ptr() + lead, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:lead] == 0xA5) and np.all(got[lead + n:] == 0xA5)
    assert np.array_equal(got[lead:lead + n].reshape(h, w, 3), oracle_image(cf, h, w, mode, qt, grids))


def _rejected_by_reference(data):
    try:
        ir.decode(data)
    except (AssertionError, IndexError, KeyError):
        return True
    return False


def _defects(data):
    """{kind: file}: the scan cut in half; the first bit from the middle of the scan on whose
    flip the reference decoder fails (bytes that are or neighbour an 0xFF are left alone), as in
    test_gpu_jpeg_interleaved._defects."""
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
    return out


@pytest.mark.parametrize('name', ['p24x40_420', 'p33x35_422'])
def test_gpu_defective_files_raise_and_leave_out_alone(name):
    import torch
    from jds import codec
    data, exp = fixture(name)
    d = ir.decode(data)
    bad = _defects(data)
    assert set(bad) == {'truncated', 'flipped'} and all(_rejected_by_reference(f) for f in bad.values())
    good = oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
    for kind, f in bad.items():
        out = torch.full((d['H'], d['W'], 3), 0x5A, dtype=torch.uint8, device='cuda')
        with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x'):
            codec.jpeg_to_rgb(f, out=out)
        assert bool((out == 0x5A).all()), kind
        with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x'):
            codec.jpeg_to_rgb(f)
        assert np.array_equal(codec.jpeg_to_rgb(data), good)        # the same pooled context


def test_gpu_defective_file_status_and_device_output_on_one_context():
    """jds_jpeg_to_rgb_render into the caller's device buffer on a leased context: a defective
    scan returns before the single-image rendering (the batch renderings would write zeros), so
    the buffer keeps its fill; info.status is the host model's word; the same context then
    renders the good file."""
    import ctypes as C
    import re
    import torch
    from jds import _abi, entropy
    lib = _abi.lib()
    data, exp = fixture('p24x40_420')
    d = ir.decode(data)
    good = oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
    with _abi.lease(0) as ctx:
        for kind, f in _defects(data).items():
            with pytest.raises(ValueError, match='defective scan data: .* \\(status 0x') as host:
                entropy.host_decode_jpeg(f)
            out = torch.full((d['H'], d['W'], 3), 0xA5, dtype=torch.uint8, device='cuda:0')
            torch.cuda.synchronize()
            for image, want in ((f, int(re.search(r'status 0x([0-9a-f]+)', str(host.value)).group(1), 16)), (data, 0)):
                a, p, n = entropy._bytes_arg(image)
                info = _abi.JpegInfo()
                rc = lib.jds_jpeg_to_rgb_render(ctx.handle, p, n, C.c_void_p(int(out.data_ptr())), out.numel(), 1, None,
                                                C.byref(info), _abi.render_code('reference'))
                assert int(info.status) == want, kind
                if want:
                    assert rc == _abi.JDS_EINVAL and bool((out == 0xA5).all()), kind
                    assert re.match(r'defective scan data: .* \(status 0x', lib.jds_last_error().decode())
                else:
                    assert rc == 0 and np.array_equal(out.cpu().numpy(), good), kind


def test_gpu_with_info():
    from jds import codec, entropy
    data, exp = fixture('p33x35_422')
    img, info = codec.jpeg_to_rgb(data, with_info=True)
    d = entropy.decode_jpeg(data)
    assert info['route'] == 'fused'
    assert np.array_equal(info['coeffs'], d['coeffs']) and np.array_equal(info['coeffs'], exp)
    assert np.array_equal(info['qtables'], d['qtables']) and info['grids'] == d['grids']
    assert (info['H'], info['W'], info['mode']) == (d['H'], d['W'], d['mode'])
    assert np.array_equal(img, codec.jpeg_to_rgb(data))
