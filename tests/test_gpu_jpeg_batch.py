"""GPU checks of the batch of foreign files (jds_jpeg_batch_to_rgb: the entropy decode over the
descriptors of many files, k_jpeg_inv_batch).  The yardstick is always the single-file call on
the same inputs (codec.jpeg_to_rgb, itself pinned to the oracle by test_gpu_jpeg_rgb), and
test_jpeg_interleaved_cpu.oracle_image where the expected coefficients are at hand."""
import re

import numpy as np
import pytest

import interleaved_ref as ir
from oracle import cpu_ref
from test_jpeg_batch_cpu import check_layout, flipped, three_table_file, tile_edge_batch
from test_jpeg_interleaved_cpu import NAMES, Q50, fixture, oracle_image, written

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def singles(files):
    from jds import codec
    return [codec.jpeg_to_rgb(f) for f in files]


def assert_batch_equals_singles(files, **kw):
    from jds import codec
    imgs, info = codec.jpeg_batch_to_rgb(files, with_info=True, **kw)
    check_layout(info['items'], info['rgb_bytes'], info['coef_entries'])
    for i, (a, b) in enumerate(zip(imgs, singles(files))):
        assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), i
    return imgs, info


@pytest.mark.parametrize('order', ['manifest', 'shuffled'])
def test_gpu_fixture_batch(order):
    names = list(NAMES)
    if order == 'shuffled':
        names = [names[i] for i in np.random.default_rng(5).permutation(len(names))]
    files = [fixture(n) for n in names]
    imgs, info = assert_batch_equals_singles([f[0] for f in files])
    for (data, exp), img in zip(files, imgs):
        d = ir.decode(data)
        assert np.array_equal(img, oracle_image(exp, d['H'], d['W'], d['mode'], d['qtables'], d['grids']))


def test_gpu_tile_edge_batch_alternating_modes():
    batch = tile_edge_batch()
    imgs, info = assert_batch_equals_singles([b[3] for b in batch])
    for (h, w, mode, data, exp, qt, grids), img in zip(batch, imgs):
        assert np.array_equal(img, oracle_image(exp, h, w, mode, qt, grids)), (h, w, mode)


def long_file():
    """185x199 4:2:0 of random_padded(amp=300, density=0.9): checked here on the CPU that its scan
    spans at least three workgroups and needs at least two rounds (enlarged if it does not)."""
    from jds import entropy
    s_bits, g = entropy.decode_info()
    h, w = 185, 199
    while True:
        data = three_table_file(h, w, '4:2:0', 31)[0]
        length = entropy.parse_jpeg(data)['scans'][0]['length']
        rounds = entropy.host_decode_jpeg(data, s_bits)[1][0]
        if 8 * length > 2 * g * s_bits and rounds >= 2:
            return data
        h, w = h + 64, w + 64
        assert h < 1000


def test_gpu_files_settle_in_different_rounds():
    """A scan of three workgroups between one-workgroup files: the batch takes the rounds of its
    slowest file, not the sum."""
    from jds import codec
    big = long_file()
    small = [fixture('p24x40_420')[0], fixture('p33x35_422')[0], written(41, 50, '4:2:0', 3)[0]]
    files = [small[0], small[1], big, small[2]]
    imgs, info = assert_batch_equals_singles(files)
    single_rounds = [codec.jpeg_to_rgb(f, with_info=True)[1]['rounds'] for f in files]
    assert single_rounds[2] >= 2 and single_rounds[0] == 1
    assert info['rounds'] >= 2 and info['rounds'] == max(single_rounds)


def test_gpu_both_restart_routes_in_one_batch():
    from jds import entropy
    lane_max = entropy.restart_info()[1]
    desc = written(112, 112, '4:2:0', 17, ri=22)[0]       # 132 blocks per interval, three intervals
    d = entropy.parse_jpeg(desc)
    assert 22 * d['mcu']['blocks'] > lane_max and -(-d['mcu']['rows'] * d['mcu']['cols'] // 22) == 3
    pad = written(150, 160, '4:2:0', 18, ri=3)[0]         # padding blocks, the lane route
    p = entropy.parse_jpeg(pad)
    assert 3 * p['mcu']['blocks'] <= lane_max
    assert p['mcu']['rows'] * p['mcu']['cols'] * 6 * 64 > p['coeffs_needed']
    lane = [fixture('p40x72_420_rst2')[0], fixture('p48x48_420_opt_rstrow')[0]]
    for f in lane:
        q = entropy.parse_jpeg(f)
        assert 0 < q['scans'][0]['restart_interval'] * q['mcu']['blocks'] <= lane_max
    plain = fixture('p24x40_420')[0]
    assert entropy.parse_jpeg(plain)['scans'][0]['restart_interval'] == 0
    assert_batch_equals_singles([lane[0], desc, plain, pad, lane[1]])


def mixed20():
    """20 files: the fixtures, writer-made files of the three modes with and without restart
    intervals, and this library's own three-scan files."""
    files = [fixture(n)[0] for n in NAMES[:8]]
    for i, (h, w, mode, ri) in enumerate([(41, 50, '4:2:0', 0), (33, 35, '4:2:2', 3), (20, 100, '4:4:4', 5),
                                          (40, 56, '4:2:0', 4), (17, 23, '4:2:0', 0), (65, 131, '4:2:2', 0),
                                          (33, 129, '4:4:4', 0), (112, 112, '4:2:0', 22)]):
        files.append(written(h, w, mode, 50 + i, ri=ri)[0])
    files += own_files()
    assert len(files) == 20
    return files


def own_files():
    """This library's own files (three non-interleaved scans), with and without restart intervals."""
    from jds import codec, entropy
    out = []
    for h, w, mode, ri in ((48, 80, '4:2:0', 0), (48, 80, '4:2:0', 64), (40, 56, '4:2:2', 0), (32, 48, '4:4:4', 64)):
        raw = codec.compress_reconstruct_raw(cpu_ref.random_image(h, w, 3 + ri), 50, Q50, mode, True, maps=False)
        if ri:
            out.append(entropy.encode_jfif(raw['coeffs'], h, w, mode, Q50, restart_interval=ri)[0])
        else:
            out.append(entropy.encode_jfif(raw['coeffs'], h, w, mode, Q50)[0])
    return out


def test_gpu_own_and_foreign_together():
    from jds import codec
    own = own_files()
    foreign = [fixture('p33x35_422')[0], written(41, 50, '4:2:0', 3)[0], fixture('p40x72_420_rst2')[0]]
    files = [own[0], foreign[0], own[1], foreign[1], own[2], foreign[2], own[3]]
    imgs, info = assert_batch_equals_singles(files)
    assert [it['interleaved'] for it in info['items']] == [False, True, False, True, False, True, False]
    for i in (0, 2, 4, 6):
        assert np.array_equal(imgs[i], codec.decompress_jfif(files[i]))


def test_gpu_permutation():
    from jds import codec
    files = mixed20()
    ref = codec.jpeg_batch_to_rgb(files)
    for a, b in zip(ref, singles(files)):
        assert np.array_equal(a, b)
    perm = np.random.default_rng(11).permutation(len(files))
    got = codec.jpeg_batch_to_rgb([files[i] for i in perm])
    for k, i in enumerate(perm):
        assert np.array_equal(got[k], ref[i]), (k, i)


def test_gpu_output_on_the_device_with_guards():
    import torch
    from jds import codec
    files = [b[3] for b in tile_edge_batch()[::2]] + [fixture(n)[0] for n in NAMES[:3]]
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    buf = torch.full((rgb_bytes + 512,), 0xA5, dtype=torch.uint8, device='cuda')
    views = codec.jpeg_batch_to_rgb(files, out=buf[256:256 + rgb_bytes])
    got = buf.cpu().numpy()
    assert np.all(got[:256] == 0xA5) and np.all(got[256 + rgb_bytes:] == 0xA5)
    for it, v, ref in zip(items, views, singles(files)):
        assert v.device.type == 'cuda' and v.data_ptr() == buf.data_ptr() + 256 + it['rgb_off']
        assert np.array_equal(v.cpu().numpy(), ref)
        end = 256 + it['rgb_off'] + ref.size
        assert np.all(got[end:256 + -(-(it['rgb_off'] + ref.size) // 256) * 256] == 0xA5)
        assert np.array_equal(got[256 + it['rgb_off']:end].reshape(ref.shape), ref)
    own = codec.jpeg_batch_to_rgb(files, out='device')
    assert all(o.device.type == 'cuda' and np.array_equal(o.cpu().numpy(), r) for o, r in zip(own, singles(files)))
    assert own[1].data_ptr() - own[0].data_ptr() == items[1]['rgb_off']
    with pytest.raises(ValueError, match=f'image buffer too small: {rgb_bytes} bytes needed'):
        codec.jpeg_batch_to_rgb(files, out=buf[:rgb_bytes - 1])
    with pytest.raises(ValueError, match='out must be'):
        codec.jpeg_batch_to_rgb(files, out=buf.reshape(2, -1))


def test_gpu_errors_in_the_middle():
    from jds import codec
    good = [fixture('p33x35_422')[0], fixture('p31x45_420_q95_opt')[0], written(41, 50, '4:2:0', 3)[0]]
    bad = flipped(fixture('p24x40_420')[0])
    with pytest.raises(ValueError, match=r'defective scan data: .* \(status 0x') as e:
        codec.jpeg_to_rgb(bad)
    st = int(re.search(r'status 0x([0-9a-f]+)', str(e.value)).group(1), 16)
    files = [good[0], bad, good[1], b'not a jpeg', good[2]]
    imgs, info = codec.jpeg_batch_to_rgb(files, errors='return', with_info=True)
    assert imgs[1] is None and imgs[3] is None
    assert [it['status'] for it in info['items']] == [0, st, 0, 0, 0]
    assert info['items'][3]['rc'] != 0 and info['items'][3]['rgb_off'] == -1 and info['items'][1]['rc'] == 0
    for i, ref in zip((0, 2, 4), singles(good)):
        assert np.array_equal(imgs[i], ref)
    # the defective file's region is all zero (host output: read it through the layout)
    import torch
    buf = torch.full((info['rgb_bytes'],), 0xA5, dtype=torch.uint8, device='cuda')
    codec.jpeg_batch_to_rgb(files, out=buf, errors='return')
    it = info['items'][1]
    assert bool((buf[it['rgb_off']:it['rgb_off'] + it['H'] * it['W'] * 3] == 0).all())
    with pytest.raises(ValueError, match='^file 1: defective scan data'):
        codec.jpeg_batch_to_rgb(files)
    with pytest.raises(ValueError, match='^file 1: '):
        codec.jpeg_batch_to_rgb([good[0], b'not a jpeg', good[1]])
    assert codec.jpeg_batch_to_rgb([]) == []
    assert codec.jpeg_batch_to_rgb([b'not a jpeg'], errors='return') == [None]


def test_gpu_context_buffers_are_reused():
    """A large batch, a small one, the large one again on one leased context."""
    from jds import codec, _abi
    large, small = mixed20(), [fixture('p17x23_420')[0], fixture('p33x35_422')[0]]
    with _abi.lease(0) as ctx:
        pass                                    # the pool hands the same context to the calls below
    a = codec.jpeg_batch_to_rgb(large)
    assert _abi.pool_size(0) >= 1
    b = codec.jpeg_batch_to_rgb(small)
    c = codec.jpeg_batch_to_rgb(large)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    assert all(np.array_equal(x, y) for x, y in zip(a, singles(large)))
    assert all(np.array_equal(x, y) for x, y in zip(b, singles(small)))
