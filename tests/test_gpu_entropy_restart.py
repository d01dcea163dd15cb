"""Restart intervals on the GPU: the writer at interval 64 (jds_encode_jfif_rst,
jds_plan_entropy_rst) against tests/restart_ref.py byte for byte, the
one-lane-per-interval decode (k_dec_rst) through jds_decode_jfif /
jds_decompress_jfif for the writer's and other intervals, the descriptor route
for intervals too long for a lane, both byte sources of the lanes, and the
asynchronous device-resident batch (jds_plan_entropy_decode_rst) with its
verdicts on damaged files."""
import functools

import numpy as np
import pytest

import restart_ref as rr
from oracle import cpu_ref
from oracle import jpeg_entropy as je
from test_entropy_decode_cpu import extreme_coeffs

pytestmark = pytest.mark.gpu

ONES = np.ones((8, 8))


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


@functools.lru_cache(maxsize=None)
def codec_coeffs(h, w, mode, q):
    img = cpu_ref.random_image(h, w, 3)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, mode != '4:4:4', metrics=False)
    return np.asarray(ref['coeffs'], np.int16).reshape(-1), np.asarray(ref['qtable'], np.float64)


def strip_coeffs(n, seed):
    """8 x 8n at 4:4:4: n blocks per scan -- sparse DC steps, a few dense and a few no-EOB blocks."""
    rng = np.random.default_rng(seed)
    blk = np.zeros((3 * n, 64), np.int64)
    pick = rng.choice(len(blk), max(1, len(blk) // 5), replace=False)
    blk[pick, 0] = rng.integers(-300, 301, len(pick))
    for i in rng.choice(len(blk), max(1, len(blk) // 11), replace=False):
        blk[i, 1:] = rng.integers(-60, 61, 63)
    for i in rng.choice(len(blk), max(1, len(blk) // 13), replace=False):
        blk[i, 63] = rng.choice([-1, 1, 700])
    return blk.astype(np.int16).reshape(-1)


def _writer_equals_reference(cf, h, w, mode, qt):
    from jds import entropy
    ref, ref_bits, nm = rr.encode_jfif_rst(cf, h, w, mode, qt, 64)
    data, bits = entropy.encode_jfif(cf, h, w, mode, qt, restart_interval=64)
    assert len(data) == len(ref) and data == ref
    assert bits == ref_bits
    d = entropy.decode_jfif(data)
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] == 0
    assert (d['H'], d['W'], d['mode']) == (h, w, mode)
    return ref, nm


def test_restart_info_and_unsupported_intervals():
    from jds import entropy
    wi, lm = entropy.restart_info()
    assert wi == 64 and lm >= 64
    cf, qt = codec_coeffs(16, 16, '4:2:0', 1)
    with pytest.raises(ValueError, match='64'):
        entropy.encode_jfif(cf, 16, 16, '4:2:0', qt, restart_interval=32)


@pytest.mark.parametrize('h,w,mode,q,markers', [(64, 96, '4:2:0', 50, 1), (16, 16, '4:2:0', 1, 0),
                                                (2, 2, '4:2:0', 50, 0), (264, 200, '4:2:2', 95, 24)])
def test_gpu_writer_equals_reference_codec_frames(h, w, mode, q, markers):
    cf, qt = codec_coeffs(h, w, mode, q)
    ref, nm = _writer_equals_reference(cf, h, w, mode, qt)
    assert nm == markers
    if markers == 24:
        # 825 luma blocks: 13 intervals (RSTm wraps past 7, the last interval ragged), 429 chroma: 7 each
        assert rr.counts(h, w, mode) == (825, 429)
        assert b'\xff\xd0' in ref and ref.count(b'\xff\xd7') >= 1
        assert rr.stuffed_ff_before_marker(ref) >= 1  # a stuffed 0xFF ends an interval


def test_gpu_writer_equals_reference_extreme_coefficients():
    """Category-11 DC differences at interval starts, ZRL runs, +-1023 AC, blocks without EOB."""
    cf = extreme_coeffs(96, 128, 1)
    ref, nm = _writer_equals_reference(cf, 96, 128, '4:4:4', ONES)
    assert nm == 3 * 2
    assert rr.stuffed_ff_before_marker(ref) >= 1


@pytest.mark.parametrize('n', [63, 64, 65, 129])
def test_gpu_writer_equals_reference_interval_counts_around_the_wave_size(n):
    _writer_equals_reference(strip_coeffs(n, n), 8, 8 * n, '4:4:4', ONES)


@pytest.mark.parametrize('h,w,mode', [(33, 47, '4:4:4'), (64, 96, '4:2:2')])
@pytest.mark.parametrize('ri', [1, 7, 100])
def test_gpu_decodes_reference_files_of_other_intervals(h, w, mode, ri):
    from jds import entropy
    cf, qt = codec_coeffs(h, w, mode, 50)
    d = entropy.decode_jfif(rr.encode_jfif_rst(cf, h, w, mode, qt, ri)[0])
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] == 0


def test_gpu_interval_longer_than_a_lane_takes_the_descriptor_route():
    """Ri = lane_max_blocks + 1 on a strip of Ri + 1 blocks per scan: two intervals per scan, each a
    descriptor of the self-synchronising kernels."""
    from jds import entropy
    lm = entropy.restart_info()[1]
    n = lm + 2
    cf = strip_coeffs(n, 5)
    data = rr.encode_jfif_rst(cf, 8, 8 * n, '4:4:4', ONES, lm + 1)[0]
    assert [s['restart_interval'] for s in entropy.parse_jfif(data)['scans']] == [lm + 1] * 3
    d = entropy.decode_jfif(data)
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] >= 1


def test_gpu_round_trip_1080p_and_decompress():
    from jds import codec, entropy
    h, w, mode, q = 1080, 1920, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 9)
    qt = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)
    raw = codec.compress_reconstruct_raw(img, q, qt, mode, True, maps=False)
    data, _ = entropy.encode_jfif(raw['coeffs'], h, w, mode, qt, restart_interval=64)
    d = entropy.decode_jfif(data)
    assert np.array_equal(d['coeffs'], np.asarray(raw['coeffs'], np.int16).reshape(-1)) and d['rounds'] == 0
    assert np.array_equal(codec.decompress_jfif(data), raw['reconstructed'])


def test_gpu_all_zero_4k_is_one_pass():
    """The frame the plain decoder settles one subsequence at a time."""
    from jds import entropy
    h, w, mode = 2160, 3840, '4:4:4'
    ny, nc = rr.counts(h, w, mode)
    cf = np.zeros(64 * (ny + 2 * nc), np.int16)
    plain, _ = entropy.encode_jfif(cf, h, w, mode, ONES)
    data, bits = entropy.encode_jfif(cf, h, w, mode, ONES, restart_interval=64)
    # from the reference on one interval: 64 zero blocks are 64 * 6 (luma) or 64 * 4 (chroma) bits,
    # whole bytes without an 0xFF, so an interval adds nothing but its marker's two bytes
    z = np.zeros((64, 64), np.int16)
    for chroma, per in ((False, 6), (True, 4)):
        seg, nb = je.encode_scan(z, chroma)
        assert nb == 64 * per and len(seg) == 8 * per and 0xFF not in seg
    assert ny % 64 == 0 and nc % 64 == 0
    markers = (ny // 64 - 1) + 2 * (nc // 64 - 1)
    assert len(data) == len(plain) + 6 + 2 * markers
    assert bits == [6 * ny, 4 * nc, 4 * nc]
    d = entropy.decode_jfif(data)
    assert d['rounds'] == 0 and d['coeffs'].size == cf.size and not d['coeffs'].any()


def test_gpu_lanes_read_intervals_shorter_than_their_row():
    """k_dec_rst reads bytes one way, through a 128-byte row per lane.  64 x 96 at 4:4:4, Ri = 4:
    72 intervals of at most 101 bytes, each inside its lane's first row (no refill; ragged ends
    on both sides of the row's aligned dwords)."""
    from jds import entropy
    cf, qt = codec_coeffs(64, 96, '4:4:4', 50)
    blocks = cf.reshape(-1, 64)
    longest = max(len(seg) for k in range(3) for seg, _ in rr.scan_intervals(blocks[96 * k:96 * (k + 1)], k > 0, 4))
    assert longest + 3 + 16 <= 128  # whatever the interval's alignment in memory
    d = entropy.decode_jfif(rr.encode_jfif_rst(cf, 64, 96, '4:4:4', qt, 4)[0])
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] == 0


def test_gpu_lanes_refill_their_rows_over_dense_intervals():
    """8 x 32768 at 4:4:4 with every AC coefficient +-1023: 64 intervals per scan of about 13 KB
    each (the densest baseline can code), a hundred row refills per lane and a workgroup's range
    of 800 KB: nothing of it can be staged at once."""
    from jds import entropy
    n = 4096
    rng = np.random.default_rng(4)
    blk = rng.choice(np.array([-1023, 1023], np.int16), (3 * n, 64))
    blk[:, 0] = 0
    cf = blk.reshape(-1)
    data, _ = entropy.encode_jfif(cf, 8, 8 * n, '4:4:4', ONES, restart_interval=64)
    scans = entropy.parse_jfif(data)['scans']
    assert all(s['length'] // 64 > 10000 for s in scans)
    d = entropy.decode_jfif(data)
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] == 0


def test_gpu_plain_files_still_take_the_self_synchronising_route():
    from jds import entropy
    h, w, mode = 264, 200, '4:2:2'
    cf, qt = codec_coeffs(h, w, mode, 95)
    ny, nc = rr.counts(h, w, mode)
    d = entropy.decode_jfif(je.encode_jfif(cf, h, w, mode, qt, ny, nc)[0])
    assert np.array_equal(d['coeffs'], cf) and d['rounds'] >= 1


# ------------------------------------------------------------- plan batch --

def _batch():
    import torch
    from jds import _abi, codec, entropy
    H, W, mode, q, n = 264, 200, '4:2:2', 75, 5
    frames = np.stack([cpu_ref.random_image(H, W, 300 + s) for s in range(n)])
    qt = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)
    params = [_abi.make_params(q, qt, mode, True, codec.gaussian_kernel3())] * n
    plan = _abi.Plan(_abi.context(0), params, H, W)
    ent = entropy.PlanEntropy(plan, 64)
    dev = torch.device('cuda:0')
    rgb = torch.from_numpy(frames).to(dev)
    out = torch.empty_like(rgb)
    cf = torch.empty((n, plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
    st = torch.zeros((n, _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    files = torch.full((n, ent.capacity), 0xA5, dtype=torch.uint8, device=dev)  # no zeroed output required
    lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    bits = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), 0, s)
    ent.run(cf.data_ptr(), files.data_ptr(), ent.capacity, lengths.data_ptr(), bits.data_ptr(), s)
    return plan, ent, cf, files, lengths, bits, s, (H, W, mode, qt)


def test_gpu_plan_restart_batch_round_trip():
    import torch
    plan, ent, cf, files, lengths, bits, s, (H, W, mode, qt) = _batch()
    n = cf.shape[0]
    cf2 = torch.full_like(cf, 77)
    status = torch.full((n,), 99, dtype=torch.int32, device=cf.device)
    ent.decode(files.data_ptr(), ent.capacity, lengths.data_ptr(), cf2.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert torch.equal(cf2, cf)
    assert ent.decode_rounds() == 0
    ln = lengths.cpu().tolist()
    assert all(0 < v <= ent.capacity for v in ln)
    ref, ref_bits, _ = rr.encode_jfif_rst(cf[2].cpu().numpy(), H, W, mode, qt, 64)
    assert files[2, :ln[2]].cpu().numpy().tobytes() == ref
    assert bits[2].cpu().tolist() == ref_bits
    plan.close()


def test_gpu_plan_restart_batch_reports_damaged_files():
    import torch
    from jds import _abi
    plan, ent, cf, files, lengths, bits, s, _ = _batch()
    torch.cuda.synchronize()
    n = cf.shape[0]
    host = files.cpu().numpy().copy()
    ln = lengths.cpu().tolist()
    lengths2 = lengths.clone()
    lengths2[1] = 0
    f2 = host[2, :ln[2]]
    m = [i for i in range(ln[2] - 1) if f2[i] == 0xFF and 0xD0 <= f2[i + 1] <= 0xD7]
    assert len(m) == 24
    host[2, m[3] + 1] = 0xD0 + ((int(f2[m[3] + 1]) - 0xD0 + 1) & 7)  # RST3 -> RST4
    f3 = host[3, :ln[3]]
    m3 = [i for i in range(ln[3] - 1) if f3[i] == 0xFF and 0xD0 <= f3[i + 1] <= 0xD7]
    # a byte inside the Y scan's fourth interval, neither an 0xFF, nor next to one, nor turned into one
    p = next(i for i in range(m3[2] + 8, m3[3] - 8) if 0xFF not in f3[i - 1:i + 2] and f3[i] ^ 0x55 != 0xFF)
    host[3, p] ^= 0x55
    files2 = torch.from_numpy(host).to(files.device)
    cf2 = torch.full_like(cf, 77)
    status = torch.full((n,), 99, dtype=torch.int32, device=cf.device)
    ent.decode(files2.data_ptr(), ent.capacity, lengths2.data_ptr(), cf2.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    sh = status.cpu().tolist()
    assert sh[0] == 0 and sh[4] == 0
    assert torch.equal(cf2[0], cf[0]) and torch.equal(cf2[4], cf[4])
    assert sh[1] == _abi.DEC_HEADER and not cf2[1].any()
    assert sh[2] == _abi.DEC_RESTART and not cf2[2].any()
    scan_defects = _abi.DEC_CODE | _abi.DEC_K63 | _abi.DEC_COUNT | _abi.DEC_OVERRUN
    assert sh[3] & scan_defects and not sh[3] & (_abi.DEC_HEADER | _abi.DEC_RESTART), sh[3]
    plan.close()
