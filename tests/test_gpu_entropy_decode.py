"""GPU checks of the JFIF decoder (csrc/jds_entropy_dec.hip): oracle-written files
back to their coefficients, encoder round trips at size, the propagation
regimes (sequential all-zero luma across workgroups, slow-synchronising dense
noise, scans shorter than one subsequence), decompression byte-equal to the
codec's own reconstruction on every inverse route, the device-resident batch
path, Huffman tables from the file, and error returns for defective scan data."""
import numpy as np
import pytest

from oracle import cpu_ref
from oracle import jpeg_entropy as je

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def counts(h, w, mode):
    ny = ((h + 7) // 8) * ((w + 7) // 8)
    sy, sx = (2, 2) if mode == '4:2:0' else ((1, 2) if mode == '4:2:2' else (1, 1))
    nc = ((h // sy + 7) // 8) * ((w // sx + 7) // 8)
    return ny, nc


def extreme_coeffs(h, w, seed):
    """test_gpu_jfif_extreme_coefficients' construction (tests/test_gpu_entropy.py)."""
    ny, nc = counts(h, w, '4:4:4')
    rng = np.random.default_rng(seed)
    blk = np.zeros((ny + 2 * nc, 64), np.int64)
    blk[:, 0] = rng.choice([1023, -1024, 0, 5], len(blk))
    zz = je.ZIGZAG
    kind = rng.integers(0, 5, len(blk))
    for i in np.flatnonzero(kind == 1):
        blk[i, zz[63]] = rng.choice([1023, -1023, 1])
    for i in np.flatnonzero(kind == 2):
        blk[i, zz[1:]] = rng.integers(-1023, 1024, 63)
    for i in np.flatnonzero(kind == 3):
        pos = rng.choice(np.arange(1, 64), 3, replace=False)
        blk[i, zz[pos]] = rng.integers(-1023, 1024, 3)
    return blk.astype(np.int16).reshape(-1)


def _check(d, cf, h, w, mode, qt):
    assert (d['H'], d['W'], d['mode']) == (h, w, mode)
    assert np.array_equal(d['qtable'], np.asarray(qt, np.float64).reshape(8, 8))
    assert d['coeffs'].dtype == np.int16
    assert np.array_equal(d['coeffs'], np.asarray(cf, np.int16).reshape(-1)), f"rounds {d['rounds']}"


@pytest.mark.parametrize('h,w,mode,q,pf', [
    (64, 96, '4:2:0', 50, True), (48, 40, '4:2:2', 90, False), (33, 47, '4:4:4', 10, False),
    (120, 160, '4:2:0', 100, True), (16, 16, '4:2:0', 1, False), (2, 2, '4:2:0', 50, False),
    (1, 9, '4:4:4', 75, False), (264, 200, '4:2:2', 95, True),
])
def test_gpu_decodes_oracle_files(h, w, mode, q, pf):
    """Independent of the GPU encoder: CPU codec coefficients, CPU-written file."""
    from jds import entropy
    img = cpu_ref.random_image(h, w, 31 * h + w + q)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, pf, metrics=False)
    ny, nc = counts(h, w, mode)
    data, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    _check(entropy.decode_jfif(data), ref['coeffs'], h, w, mode, ref['qtable'])


def test_gpu_round_trip_1080p():
    from jds import entropy
    from jds.codec import compress_reconstruct_raw
    h, w, mode, q = 1080, 1920, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 9)
    qt = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)
    raw = compress_reconstruct_raw(img, q, qt, mode, True, maps=False)
    data, _ = entropy.encode_jfif(raw['coeffs'], h, w, mode, qt)
    _check(entropy.decode_jfif(data), raw['coeffs'], h, w, mode, qt)


def test_gpu_round_trip_extreme_coefficients():
    from jds import entropy
    h, w, mode = 96, 128, '4:4:4'
    cf = extreme_coeffs(h, w, 11)
    data, _ = entropy.encode_jfif(cf, h, w, mode, np.ones((8, 8)))
    _check(entropy.decode_jfif(data), cf, h, w, mode, np.ones((8, 8)))


@pytest.mark.parametrize('nblk,seed', [(65, 1), (129, 2), (193, 5)])
def test_gpu_round_trip_short_last_segment(nblk, seed):
    from jds import entropy
    h, w, mode = 8, 8 * nblk, '4:4:4'
    ny, nc = counts(h, w, mode)
    rng = np.random.default_rng(seed)
    blk = np.zeros((ny + 2 * nc, 64), np.int64)
    pick = rng.choice(len(blk), max(1, len(blk) // 9), replace=False)
    blk[pick, 0] = rng.integers(-40, 41, len(pick))
    cf = blk.astype(np.int16).reshape(-1)
    data, _ = entropy.encode_jfif(cf, h, w, mode, np.ones((8, 8)))
    _check(entropy.decode_jfif(data), cf, h, w, mode, np.ones((8, 8)))


# ---------------------------------------------------------------- regimes --

def test_gpu_all_zero_4k_luma_is_sequential_across_workgroups():
    """Every zero luma block is 6 bits ('00' + '1010'); with 1024 = 4 (mod 6) bits per
    subsequence every wrong-phase decode falls into a stable cycle, so the scan
    settles one subsequence at a time: the inter-workgroup hand-off must run
    once per workgroup."""
    from jds import entropy
    h, w, mode = 2160, 3840, '4:4:4'
    ny, nc = counts(h, w, mode)
    cf = np.zeros(64 * (ny + 2 * nc), np.int16)
    data, bits = entropy.encode_jfif(cf, h, w, mode, np.ones((8, 8)))
    assert bits[0] == 6 * ny == 777600
    S, G = entropy.decode_info()
    nsub = -(-bits[0] // S)
    groups = -(-nsub // G)
    assert groups >= 3, (S, G)
    d = entropy.decode_jfif(data)
    assert d['rounds'] >= groups - 1, (d['rounds'], groups)
    assert d['rounds'] <= groups, (d['rounds'], groups)
    assert d['coeffs'].size == cf.size and not d['coeffs'].any(), d['rounds']


def test_gpu_dense_q95_noise_synchronises_slowly_and_exactly():
    """Blocks without EOB (k re-aligns only through EOB): many in-workgroup iterations."""
    from jds import entropy
    h, w, mode, q = 264, 200, '4:4:4', 95
    img = cpu_ref.random_image(h, w, 95)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, False, metrics=False)
    ny, nc = counts(h, w, mode)
    data, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    _check(entropy.decode_jfif(data), ref['coeffs'], h, w, mode, ref['qtable'])


def test_gpu_chroma_scans_shorter_than_one_subsequence():
    from jds import entropy
    h, w, mode, q = 16, 16, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 5)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, False, metrics=False)
    ny, nc = counts(h, w, mode)
    data, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    S, _ = entropy.decode_info()
    scans = entropy.parse_jfif(data)['scans']
    assert all(8 * s['length'] < S for s in scans[1:])
    d = entropy.decode_jfif(data)
    _check(d, ref['coeffs'], h, w, mode, ref['qtable'])
    assert d['rounds'] == 1


# ------------------------------------------------------------- decompress --

def _image(case):
    if case == 'checkerboard':
        return cpu_ref.generate_colored_checkerboard(256)
    return cpu_ref.random_image(case[0], case[1], 7 * case[0] + case[1])


@pytest.mark.parametrize('case,mode,q,pf,vs_oracle', [
    ((130, 98), '4:2:0', 50, False, True),      # certified fast inverse
    ((226, 516), '4:2:0', 10, True, False),     # coarse table: k_inv2
    ((184, 260), '4:4:4', 75, False, False),    # wave-local 4:4:4 kernel
    ((98, 196), '4:2:2', 95, False, False),
    ((33, 47), '4:4:4', 50, False, False),      # odd size
    ('checkerboard', '4:2:0', 50, False, False),  # exact ties: the tile fix-up
])
def test_gpu_decompress_equals_the_codecs_reconstruction(case, mode, q, pf, vs_oracle):
    from jds import codec, entropy
    img = _image(case)
    h, w = img.shape[:2]
    qt = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)
    raw = codec.compress_reconstruct_raw(img, q, qt, mode, pf, maps=False)
    data, _ = entropy.encode_jfif(raw['coeffs'], h, w, mode, qt)
    out, info = codec.decompress_jfif(data, with_info=True)
    assert out.shape == (h, w, 3) and out.dtype == np.uint8
    assert np.array_equal(info['coeffs'], raw['coeffs'])
    assert np.array_equal(out, raw['reconstructed']), int(np.sum(out != raw['reconstructed']))
    assert np.array_equal(codec.decompress_jfif(data), out)
    if vs_oracle:
        ref = cpu_ref.compress_reconstruct(img, q, 8, mode, pf, metrics=False)
        assert np.array_equal(out, ref['reconstructed'])


# ------------------------------------------------------------- plan batch --

def test_gpu_plan_entropy_decode_batch():
    import torch
    from jds import _abi, codec, entropy
    qs = [5, 50, 95]
    H, W, mode = 360, 648, '4:2:0'
    frames = np.stack([cpu_ref.random_image(H, W, 200 + s) for s in range(len(qs))])
    params = [_abi.make_params(q, cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q), mode, True,
                               codec.gaussian_kernel3()) for q in qs]
    plan = _abi.Plan(_abi.context(0), params, H, W)
    ent = entropy.PlanEntropy(plan)
    dev = torch.device('cuda:0')
    n = len(qs)
    rgb = torch.from_numpy(frames).to(dev)
    out = torch.empty_like(rgb)
    cf = torch.empty((n, plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
    st = torch.zeros((n, _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    files = torch.zeros((n, ent.capacity), dtype=torch.uint8, device=dev)
    lengths = torch.zeros(n, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), 0, s)
    ent.run(cf.data_ptr(), files.data_ptr(), ent.capacity, lengths.data_ptr(), 0, s)
    cf2 = torch.full_like(cf, 77)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    ent.decode(files.data_ptr(), ent.capacity, lengths.data_ptr(), cf2.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    rounds = ent.decode_rounds()
    assert status.cpu().tolist() == [0, 0, 0], rounds
    assert torch.equal(cf2, cf), rounds
    assert rounds >= 1
    # inverse only, on a plan-sized fresh output and zeroed statistics
    out2 = torch.zeros_like(rgb)
    st2 = torch.zeros_like(st)
    plan.run(rgb.data_ptr(), out2.data_ptr(), cf2.data_ptr(), st2.data_ptr(), _abi.RUN_INV, s)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    sth = st2.cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1)
    assert np.all(sth['total_coeffs'] == plan.geometry.coeffs_per_frame) and np.all(sth['pixels'] == H * W)
    assert not sth['nonzero'].any() and not sth['hist'].any()
    # one frame marked uncodable (lengths[i] == 0): skipped with a status bit, the others decode
    lengths2 = lengths.clone()
    lengths2[1] = 0
    cf3 = torch.full_like(cf, 55)
    status.fill_(99)
    ent.decode(files.data_ptr(), ent.capacity, lengths2.data_ptr(), cf3.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    sh = status.cpu().tolist()
    assert sh[0] == 0 and sh[2] == 0 and sh[1] == _abi.DEC_HEADER
    assert torch.equal(cf3[0], cf[0]) and torch.equal(cf3[2], cf[2])
    assert not cf3[1].any()
    # a header that is not the plan's (another frame's table) is refused the same way
    files2 = files.clone()
    files2[0, :ent.capacity] = files[2, :ent.capacity]
    lengths3 = lengths.clone()
    lengths3[0] = lengths[2]
    status.fill_(99)
    ent.decode(files2.data_ptr(), ent.capacity, lengths3.data_ptr(), cf3.data_ptr(), status.data_ptr(), s)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_abi.DEC_HEADER, 0, 0]
    plan.close()


# ----------------------------------------------------- tables, defects --

def test_gpu_decodes_with_the_files_own_huffman_tables(monkeypatch):
    from jds import entropy
    h, w, mode, q = 64, 96, '4:2:0', 50
    img = cpu_ref.random_image(h, w, 3)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, True, metrics=False)
    ny, nc = counts(h, w, mode)
    plain, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    ac_l, ac_c, dc_l, dc_c = je.AC_LUMA, je.AC_CHROMA, je.DC_LUMA, je.DC_CHROMA
    monkeypatch.setattr(je, 'AC_LUMA', ac_c)
    monkeypatch.setattr(je, 'AC_CHROMA', ac_l)
    monkeypatch.setattr(je, 'DC_LUMA', dc_c)
    monkeypatch.setattr(je, 'DC_CHROMA', dc_l)
    data, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    assert data != plain
    _check(entropy.decode_jfif(data), ref['coeffs'], h, w, mode, ref['qtable'])


def test_gpu_defective_scan_data_is_an_error_return():
    """Error handling only: reads are bounded by the scan's byte range by construction."""
    from jds import entropy
    h, w, mode, q = 33, 47, '4:4:4', 50
    img = cpu_ref.random_image(h, w, 3)
    ref = cpu_ref.compress_reconstruct(img, q, 8, mode, False, metrics=False)
    ny, nc = counts(h, w, mode)
    data, _ = je.encode_jfif(ref['coeffs'], h, w, mode, ref['qtable'], ny, nc)
    s = entropy.parse_jfif(data)['scans'][0]
    cut = data[:s['offset'] + s['length'] // 2] + b'\xff\xd9'
    with pytest.raises(ValueError):
        entropy.decode_jfif(cut)
    cut2 = data[:s['offset'] + s['length'] // 2] + data[s['offset'] + s['length']:]
    with pytest.raises(ValueError, match='defective scan data'):
        entropy.decode_jfif(cut2)
    _check(entropy.decode_jfif(data), ref['coeffs'], h, w, mode, ref['qtable'])
    stuffed = data[:s['offset']] + b'\xff\x00' * 8 + data[s['offset'] + 16:]
    with pytest.raises(ValueError, match='defective scan data'):
        entropy.decode_jfif(stuffed)
    _check(entropy.decode_jfif(data), ref['coeffs'], h, w, mode, ref['qtable'])
