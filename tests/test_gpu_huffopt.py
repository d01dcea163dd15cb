"""Optimised Huffman tables on the GPU (jds_encode_jfif_opt, jds_plan_entropy_opt;
DESIGN.md "Optimised tables"): files byte for byte against tests/huffopt_ref.py,
plain and with restart interval 64, on coefficient sets that reach the table
builder's and the coder's corners (one-bit codes, no EOB, ZRL, extreme
coefficients, the K.3 limiter, workgroups that span frames); k_ent_opt_tables
alone on histograms no small frame produces; the decode routes that read the
files; and the standard route after an optimised call on the same context."""
import functools

import numpy as np
import pytest

import huffopt_ref as hr
import restart_ref as rr
from oracle import cpu_ref
from oracle import jpeg_entropy as je
from test_entropy_decode_cpu import extreme_coeffs

pytestmark = pytest.mark.gpu

ONES = np.ones((8, 8))
Q50 = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50)
FIB17_EOB144 = hr.steep_ac_histogram([int(v) for v in hr.fibonacci(17)[:17]], 10)
FIB17_EOB233 = hr.steep_ac_histogram([int(v) for v in hr.fibonacci(17)[:17]], 11)
FIB13_EOB34 = hr.steep_ac_histogram([int(v) for v in hr.fibonacci(13)[:13]], 7)


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def _zz(blocks_zz):
    out = np.zeros(blocks_zz.shape, np.int16)
    out[:, je.ZIGZAG] = blocks_zz
    return out.reshape(-1)


def sparse_frame(nblocks, seed):
    rng = np.random.default_rng(seed)
    zz = np.zeros((nblocks, 64), np.int64)
    zz[:, 0] = np.cumsum(rng.integers(-40, 41, nblocks))
    for b in range(nblocks):
        k = rng.choice(np.arange(1, 64), int(rng.integers(0, 12)), replace=False)
        zz[b, k] = rng.integers(-30, 31, len(k))
    return _zz(zz)


def no_eob_frame(nblocks, seed):
    zz = np.zeros((nblocks, 64), np.int64)
    zz[:, [0, 5, 63]] = np.random.default_rng(seed).integers(1, 9, (nblocks, 3))
    return _zz(zz)


def zrl_frame(nblocks, seed):
    """Runs of 16, 17, 31, 32 and 47 zeros before a coefficient, and one at position 63 after 61."""
    rng = np.random.default_rng(seed)
    zz = np.zeros((nblocks, 64), np.int64)
    for b in range(nblocks):
        pos = 1 + int(rng.choice([16, 17, 31, 32, 47, 61]))
        zz[b, pos] = int(rng.integers(1, 200)) * (-1) ** b
        if pos + 17 < 64 and b % 3 == 0:
            zz[b, pos + 17] = -3
        zz[b, 0] = b % 7
    return _zz(zz)


def limiter_frame(ny, nc, hist, seed):
    return np.concatenate([hr.blocks_with_ac_histogram(ny, hist).reshape(-1), sparse_frame(2 * nc, seed)])


@functools.lru_cache(maxsize=None)
def frame_set(name):
    """(coeffs, H, W, mode, qtable)"""
    if name == 'one_block_eob':          # one DC symbol, EOB alone: every code one bit
        zz = np.zeros((3, 64), np.int64)
        zz[:, 0] = [5, -3, -3]
        return _zz(zz), 8, 8, '4:4:4', ONES
    if name == 'one_block_two_ac':       # one DC symbol, two AC symbols per table
        zz = np.zeros((3, 64), np.int64)
        zz[:, 0] = [5, -3, -3]
        zz[:, 1] = [3, 1, -1]
        return _zz(zz), 8, 8, '4:4:4', ONES
    if name == 'all_zero':
        return np.zeros(3 * 45 * 64, np.int16), 40, 72, '4:4:4', Q50
    if name == 'no_eob':
        return no_eob_frame(3 * 45, 1), 40, 72, '4:4:4', Q50
    if name == 'zrl':
        return zrl_frame(3 * 45, 2), 40, 72, '4:4:4', Q50
    if name == 'extreme':                # DC category 11, AC category 10, ZRL runs, blocks without EOB
        return extreme_coeffs(96, 128, 1), 96, 128, '4:4:4', ONES
    if name == 'limiter':                # 169 luma blocks whose AC histogram is the 17-symbol Fibonacci one
        return limiter_frame(169, 169, FIB17_EOB144, 3), 104, 104, '4:4:4', Q50
    if name == 'sparse_420':             # 13 luma segments' worth: several segments per scan
        ny, nc = hr.counts(136, 200, '4:2:0')
        return sparse_frame(ny + 2 * nc, 4), 136, 200, '4:2:0', Q50
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, ri):
    cf, h, w, mode, qt = frame_set(name)
    return hr.encode_jfif_opt(cf, h, w, mode, qt, ri)


SETS = ('one_block_eob', 'one_block_two_ac', 'all_zero', 'no_eob', 'zrl', 'extreme', 'limiter', 'sparse_420')


@pytest.mark.parametrize('ri', [0, 64])
@pytest.mark.parametrize('name', SETS)
def test_gpu_writer_equals_reference(name, ri):
    from jds import entropy
    cf, h, w, mode, qt = frame_set(name)
    ref, ref_bits, tabs = reference(name, ri)
    data, bits = entropy.encode_jfif(cf, h, w, mode, qt, restart_interval=ri, optimize=True)
    assert len(data) == len(ref) and data == ref
    assert bits == ref_bits
    if name == 'one_block_eob':
        assert all(t[0] == [1] + [0] * 15 and len(t[1]) == 1 for t in tabs.values())
    if name == 'all_zero':
        assert [t[1] for t in tabs.values()] == [[0]] * 4              # DC category 0 and EOB
    if name == 'no_eob':
        assert 0x00 not in tabs['ac0'][1] and 0x00 not in tabs['ac1'][1]
    if name == 'zrl':
        assert 0xF0 in tabs['ac0'][1] and 0xF0 in tabs['ac1'][1]
    if name == 'extreme':
        assert 11 in tabs['dc0'][1] and any(s & 15 == 10 for s in tabs['ac0'][1])
    if name == 'limiter':
        ny = 169
        freq = hr.histograms(cf, h, w, mode, ri)['ac0']
        assert hr.unconstrained_length(freq) == 17 and tabs['ac0'][0] == [1] * 14 + [0, 3]   # K.3 ran
        assert int(freq.sum()) == 6763 and ny * 63 >= 6763


@pytest.mark.parametrize('name', ['all_zero', 'zrl', 'limiter'])
def test_gpu_optimised_files_decode_to_their_coefficients(name):
    from jds import codec, entropy
    cf, h, w, mode, qt = frame_set(name)
    ny, nc = hr.counts(h, w, mode)
    std = je.encode_jfif(cf, h, w, mode, qt, ny, nc)[0]
    for ri in (0, 64):
        data = reference(name, ri)[0]
        d = entropy.decode_jfif(data)
        assert np.array_equal(d['coeffs'], cf) and (d['H'], d['W'], d['mode']) == (h, w, mode)
        assert np.array_equal(entropy.decode_jpeg(data)['coeffs'], cf)
    # one batch that mixes optimised and standard files: the same coefficients, the same images
    files = [reference(name, 0)[0], std, reference(name, 64)[0], std]
    imgs = codec.jpeg_batch_to_rgb(files)
    one = codec.jpeg_to_rgb(std)
    assert all(im.shape == (h, w, 3) and np.array_equal(im, one) for im in imgs)


def test_gpu_table_kernel_equals_reference_on_given_histograms():
    from jds import entropy
    names = sorted(hr.histogram_cases())
    cases = hr.histogram_cases()
    freqs = np.stack([cases[n] for n in names] + [np.zeros(256, np.int64)])
    got = entropy.optimal_tables_dev(freqs)
    for n, g in zip(names + ['empty'], got):
        want = hr.optimal_table(cases[n]) if n != 'empty' else ([0] * 16, [], False)
        assert g == want, n
    assert got[names.index('fibonacci33')][2] and not got[names.index('fibonacci32')][2]


def test_gpu_round_trip_1080p_and_decompress():
    from jds import codec, entropy
    h, w, mode, q = 1080, 1920, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 9)
    raw = codec.compress_reconstruct_raw(img, q, Q50, mode, True, maps=False)
    cf = np.asarray(raw['coeffs'], np.int16).reshape(-1)
    for ri in (0, 64):
        data, bits = entropy.encode_jfif(cf, h, w, mode, Q50, restart_interval=ri, optimize=True)
        assert np.array_equal(entropy.decode_jfif(data)['coeffs'], cf)
        assert np.array_equal(codec.decompress_jfif(data), raw['reconstructed'])


# ------------------------------------------------------------- plan batches --

def _batch_frames(which):
    if which == '40x72':       # three segments per frame: a workgroup's four waves span two frames
        nb = 3 * 45
        frames = [sparse_frame(nb, 10), np.zeros(nb * 64, np.int16), limiter_frame(45, 45, FIB13_EOB34, 11),
                  no_eob_frame(nb, 12), zrl_frame(nb, 13)]
        return frames, 40, 72, '4:4:4'
    ny, nc = hr.counts(136, 136, '4:2:0')     # 289 + 2 x 81 blocks: nine segments per frame
    frames = [sparse_frame(ny + 2 * nc, 20), np.zeros((ny + 2 * nc) * 64, np.int16),
              limiter_frame(ny, nc, FIB17_EOB233, 21)]
    return frames, 136, 136, '4:2:0'


def _run_plan(frames, H, W, mode, ri, optimize, plan=None):
    import torch
    from jds import _abi, codec, entropy
    n = len(frames)
    if plan is None:
        plan = _abi.Plan(_abi.context(0), [_abi.make_params(50, Q50, mode, False, codec.gaussian_kernel3())] * n, H, W)
    ent = entropy.PlanEntropy(plan, ri, optimize=optimize)
    dev = torch.device('cuda:0')
    cf = torch.from_numpy(np.stack(frames)).to(dev)
    assert cf.shape[1] == plan.geometry.coeffs_per_frame
    files = torch.full((n, ent.capacity), 0xA5, dtype=torch.uint8, device=dev)  # no zeroed output required
    lengths = torch.full((n,), -1, dtype=torch.int64, device=dev)
    bits = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ent.run(cf.data_ptr(), files.data_ptr(), ent.capacity, lengths.data_ptr(), bits.data_ptr(), s)
    torch.cuda.synchronize()
    ln = lengths.cpu().tolist()
    host = files.cpu().numpy()
    return plan, ent, cf, files, lengths, [host[i, :max(ln[i], 0)].tobytes() for i in range(n)], ln, bits.cpu().tolist()


@pytest.mark.parametrize('ri', [0, 64])
@pytest.mark.parametrize('which', ['40x72', '136x136'])
def test_gpu_plan_batches_whose_workgroups_span_frames(which, ri):
    import torch
    from jds import _abi, entropy
    frames, H, W, mode = _batch_frames(which)
    assert len({f.tobytes() for f in frames}) == len(frames)
    refs = [hr.encode_jfif_opt(f, H, W, mode, Q50, ri) for f in frames]
    assert len({tuple(map(tuple, r[2]['ac0'][:2])) for r in refs}) == len(frames)   # every frame its own table
    if which == '136x136':
        assert hr.unconstrained_length(hr.histograms(frames[2], H, W, mode, ri)['ac0']) == 17
    plan, ent, cf, files, lengths, data, ln, bits = _run_plan(frames, H, W, mode, ri, True)
    std_cap = entropy.PlanEntropy(plan, ri).capacity
    assert ent.capacity > std_cap                      # 1665 against 1660 bits per block
    for i, (ref, ref_bits, _) in enumerate(refs):
        assert ln[i] == len(ref) and data[i] == ref, i
        assert bits[i] == ref_bits, i
    # the plan's decoder compares headers with its own: optimised files are JDS_DEC_HEADER, nothing else
    cf2 = torch.full_like(cf, 77)
    status = torch.full((len(frames),), 99, dtype=torch.int32, device=cf.device)
    s = torch.cuda.current_stream().cuda_stream
    ent.decode(files.data_ptr(), ent.capacity, lengths.data_ptr(), cf2.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_abi.DEC_HEADER] * len(frames)
    # the standard route on the same plan after the optimised one: today's files
    ny, nc = hr.counts(H, W, mode)
    _, _, _, _, _, sdata, sln, sbits = _run_plan(frames, H, W, mode, ri, False, plan)
    for i, f in enumerate(frames):
        want = rr.encode_jfif_rst(f, H, W, mode, Q50, 64)[:2] if ri else je.encode_jfif(f, H, W, mode, Q50, ny, nc)
        assert sdata[i] == want[0] and sbits[i] == want[1], i
    plan.close()


@pytest.mark.parametrize('ri', [0, 64])
def test_gpu_one_uncodable_frame_in_a_batch(ri):
    frames, H, W, mode = _batch_frames('40x72')
    frames = frames[:3]
    bad = frames[1].copy().reshape(-1, 64)
    bad[7, 0] = 3000                                   # DC differences of category 12
    bad[50, 9] = -2000                                 # AC category 11
    frames[1] = bad.reshape(-1)
    plan, ent, cf, files, lengths, data, ln, bits = _run_plan(frames, H, W, mode, ri, True)
    assert ln[1] == 0 and ln[0] > 0 and ln[2] > 0
    for i in (0, 2):
        ref, ref_bits, _ = hr.encode_jfif_opt(frames[i], H, W, mode, Q50, ri)
        assert data[i] == ref and bits[i] == ref_bits
    plan.close()


@pytest.mark.parametrize('name', ['zrl', 'sparse_420'])
def test_gpu_standard_route_unchanged_after_an_optimised_call(name):
    """Same process, same pooled context: optimised, then standard -- stale per-frame state would show."""
    from jds import entropy
    cf, h, w, mode, qt = frame_set(name)
    ny, nc = hr.counts(h, w, mode)
    for ri in (0, 64):
        assert entropy.encode_jfif(cf, h, w, mode, qt, restart_interval=ri, optimize=True)[0] == reference(name, ri)[0]
        data, bits = entropy.encode_jfif(cf, h, w, mode, qt, restart_interval=ri)
        want = rr.encode_jfif_rst(cf, h, w, mode, qt, 64)[:2] if ri else je.encode_jfif(cf, h, w, mode, qt, ny, nc)
        assert data == want[0] and bits == want[1]


def test_gpu_optimised_interval_must_be_the_writers():
    from jds import entropy
    cf, h, w, mode, qt = frame_set('all_zero')
    with pytest.raises(ValueError, match='64'):
        entropy.encode_jfif(cf, h, w, mode, qt, restart_interval=32, optimize=True)
