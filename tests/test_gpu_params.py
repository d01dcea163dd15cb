"""Plans, the context path and the subsample stage on tables and taps other
than the defaults (params_cases.py), against params_ref (the oracle's stage
functions with the table and the taps as arguments).

The table's DC step alone routes the inverse (k_inv2 above 60, the certified
kernel otherwise, coarse items of a mixed plan seeded into its exact mode), the
taps' signs and sum switch the full run's fixed |q Q| <= 1152 certificate, and
Q and the taps set the forward's certification limits.  Every route must give
the reference's coefficients, bytes and statistics: the default run, the exact
kernels (JDS_RUN_EXACT), the certified ones asked for and with every tile or
block recomputed (FIXALL), the SSE run, the two phases as two calls.  Where
the taps' sum is not 1 every chroma block takes the forward's exact fix-up;
asymmetric and non-finite taps are refused."""
import functools

import numpy as np
import pytest

import params_ref
from oracle import cpu_ref
from params_cases import BAD_TAPS, TABLES, TAPS, apriori_ok, sign_frames
from test_gpu_inv_fast import _coarse_frames, _params, _plan, _same

pytestmark = pytest.mark.gpu

DMAX = 1152
STAT_FIELDS = ('nonzero', 'magnitude_bits', 'hist', 'total_coeffs')


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


@functools.lru_cache(maxsize=None)
def _frame(kind, h, w):
    if kind == 'random':
        return cpu_ref.random_image(h, w, 2300 + h + w)
    if kind in ('prim', 'half'):
        return _coarse_frames(h, w, 2301)[1 if kind == 'prim' else 2]
    if kind == 'gray':
        return np.full((h, w, 3), 128, np.uint8)
    if kind in ('cb_sign', 'cr_sign'):
        return np.ascontiguousarray(sign_frames(h, w)[kind == 'cr_sign'])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _ref(kind, h, w, table, mode, pf, taps, bs=8):
    """params_ref's result for one item, computed once per session and left unchanged."""
    return params_ref.compress_reconstruct(_frame(kind, h, w), TABLES[table], mode, pf,
                                           TAPS[taps or 'gauss075'], bs)


def _items(tables, taps=None, bs=8):
    return [(TABLES[t], None if taps is None else TAPS[taps], bs) for t in tables]


def _equals_ref(run, refs, frames, h, w, bs=8, sse=False):
    """Coefficients, bytes, hist, nonzero, total_coeffs and magnitude_bits of every item."""
    out, cf, st, _ = run
    overhead = 2 * -(-h // bs) * -(-w // bs)
    for i, ref in enumerate(refs):
        assert np.array_equal(cf[i], ref['coeffs']), (i, int(np.sum(cf[i] != ref['coeffs'])))
        assert np.array_equal(out[i], ref['reconstructed']), (i, int(np.sum(out[i] != ref['reconstructed'])))
        assert [int(v) for v in st[i]['hist']] == [int(v) for v in ref['hist']], i
        nz = int(st[i]['nonzero'])
        assert nz == ref['bitrate']['nonzero_count'], i
        assert int(st[i]['total_coeffs']) == ref['bitrate']['total_coeffs'], i
        # estimate_bitrate_no_entropy: overhead + 6 per nonzero + sum(ceil(log2(|q| + 1)) + 1)
        assert overhead + 6 * nz + int(st[i]['magnitude_bits']) == ref['bitrate']['estimated_bits'], i
        if sse:
            d = frames[i].astype(np.int64) - ref['reconstructed'].astype(np.int64)
            assert int(st[i]['sse_rgb']) == int((d * d).sum()), i


def _agree(runs):
    for r in runs[1:]:
        _same(r, runs[0])
        for f in STAT_FIELDS:
            assert np.array_equal(r[2][f], runs[0][2][f]), f


def _two_calls(frames, items, mode, pf):
    """JDS_RUN_FWD then JDS_RUN_INV as two calls on one plan."""
    import torch
    from jds import _abi
    H, W = frames.shape[1:3]
    plan = _abi.Plan(_abi.context(0), [_params(it, mode, pf) for it in items], H, W)
    dev = torch.device('cuda:0')
    rgb = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    out = torch.zeros_like(rgb)
    cf = torch.empty((len(items), plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
    st = torch.zeros((len(items), _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), _abi.RUN_FWD, 0)
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), _abi.RUN_INV, 0)
    torch.cuda.synchronize()
    res = (out.cpu().numpy(), cf.cpu().numpy(), st.cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1),
           plan.fix_counts())
    plan.close()
    return res


def _consecutive(frames, item, mode, pf, flags=0):
    """One single-item plan, one run per frame: [(out, cf, stats, fix)]."""
    import torch
    from jds import _abi
    H, W = frames[0].shape[:2]
    plan = _abi.Plan(_abi.context(0), [_params(item, mode, pf)], H, W)
    dev = torch.device('cuda:0')
    res = []
    for f in frames:
        rgb = torch.from_numpy(np.ascontiguousarray(f[None])).to(dev)
        out = torch.zeros_like(rgb)
        cf = torch.empty((1, plan.geometry.coeffs_per_frame), dtype=torch.int16, device=dev)
        st = torch.zeros((1, _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), flags, 0)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), cf.cpu().numpy(), st.cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1),
                    plan.fix_counts()))
    plan.close()
    return res


def _inv_tiles(h, w, mode):
    """Units of fix_counts()[1] of the 8x8 4:2:x kernel: 64 x 128 (4:2:0), 32 x 128 (4:2:2) pixel tiles."""
    return -(-h // (64 if mode == '4:2:0' else 32)) * -(-w // 128)


# ---- tables ---------------------------------------------------------------------

NAMES = sorted(TABLES)
KINDS = ('random', 'prim', 'half', 'gray')


@pytest.mark.parametrize('h,w,mode', [(64, 128, '4:2:0'), (72, 136, '4:2:0'), (32, 136, '4:2:2'), (24, 40, '4:4:4')])
def test_every_table_in_one_mixed_plan(h, w, mode):
    """DC steps from 1 to 255 in one plan: the certified inverse runs, its
    coarse items seeded into exact mode (inv_fast_any && !inv_fast_ok)."""
    from jds import _abi
    pf = mode != '4:4:4'
    assert min(TABLES[t][0, 0] for t in NAMES) <= 60 < max(TABLES[t][0, 0] for t in NAMES)
    kinds = [KINDS[i % len(KINDS)] for i in range(len(NAMES))]
    frames = np.stack([_frame(k, h, w) for k in kinds])
    refs = [_ref(k, h, w, t, mode, pf, None) for k, t in zip(kinds, NAMES)]
    runs = _plan(frames, _items(NAMES), mode, pf,
                 [0, _abi.RUN_EXACT, _abi.RUN_INV_FAST | _abi.RUN_INV_FIXALL, _abi.RUN_SSE])
    for r in runs:
        _equals_ref(r, refs, frames, h, w, sse=r is runs[3])
    _agree(runs)
    print(f'{h}x{w} {mode}: fix_counts default {runs[0][3]}, fixall {runs[2][3]}, sse {runs[3][3]}')
    if mode != '4:4:4':
        # the seeded coarse items add all their tiles to the default run's count
        coarse = sum(TABLES[t][0, 0] > 60 for t in NAMES)
        assert runs[0][3][1] >= coarse * _inv_tiles(h, w, mode)
        assert runs[2][3][1] >= len(NAMES) * _inv_tiles(h, w, mode)
    assert runs[1][3][1] == 0  # the exact kernels list nothing


def test_dc_step_above_60_takes_the_exact_inverse_whatever_the_ac_steps():
    from jds import _abi
    h, w, mode = 64, 128, '4:2:0'
    for k in ('gray', 'random'):  # gray: exact ties, which a certified kernel must list
        f = _frame(k, h, w)[None]
        dflt, fast = _plan(f, _items(['dc61_ac1']), mode, True, [0, _abi.RUN_INV_FAST])
        ref = [_ref(k, h, w, 'dc61_ac1', mode, True, None)]
        _equals_ref(dflt, ref, f, h, w)
        _equals_ref(fast, ref, f, h, w)
        assert dflt[3][1] == 0, dflt[3]  # k_inv2
        if k == 'gray':
            assert fast[3][1] > 0, fast[3]  # the certified kernel, asked for, lists the ties


def test_dc_step_60_takes_the_certified_inverse_whatever_the_ac_steps():
    """Three consecutive default runs on changing frames; an item that recomputed
    more than 1/8 of its tiles reports all of them on the next run (include/jds.h)."""
    h, w, mode = 120, 256, '4:2:0'
    kinds = ['gray', 'random', 'half']
    runs = _consecutive([_frame(k, h, w) for k in kinds], _items(['dc60_ac255'])[0], mode, True)
    nt = _inv_tiles(h, w, mode)
    for k, r in zip(kinds, runs):
        _equals_ref(r, [_ref(k, h, w, 'dc60_ac255', mode, True, None)], _frame(k, h, w)[None], h, w)
    counts = [int(r[3][1]) for r in runs]
    print(f'dc60_ac255 {h}x{w}: inverse tiles listed per run {counts} of {nt}; forward blocks '
          f'{[int(r[3][0]) for r in runs]}')
    assert counts[0] > 0  # gray-128: ties in every tile, so the certified kernel ran (k_inv2 reports 0)
    if counts[0] * 8 > nt:
        assert counts[1] == nt and counts[2] == nt, counts


def test_flat255_at_444_takes_the_wave_local_kernel():
    from jds import _abi
    h, w = 24, 40
    kinds = ['gray', 'random', 'prim']
    frames = np.stack([_frame(k, h, w) for k in kinds])
    dflt, exact = _plan(frames, _items(['flat255'] * 3), '4:4:4', False, [0, _abi.RUN_EXACT_INV])
    refs = [_ref(k, h, w, 'flat255', '4:4:4', False, None) for k in kinds]
    _equals_ref(dflt, refs, frames, h, w)
    _agree([exact, dflt])
    assert dflt[3][1] > 0 and exact[3][1] == 0  # gray-128 reconstructs to exact integers: listed


# ---- sweep plans ------------------------------------------------------------------

@pytest.mark.parametrize('h,w,mode', [(64, 128, '4:2:0'), (24, 40, '4:4:4')])
def test_sweep_plan_over_four_tables(h, w, mode):
    from jds import _abi
    pf = mode != '4:4:4'
    tabs = ['flat1', 'chroma50', 'dc61_ac1', 'rand_a']
    kinds = ['random', 'half']
    frames = np.stack([_frame(k, h, w) for k in kinds])
    refs = [_ref(k, h, w, t, mode, pf, None) for k in kinds for t in tabs]
    per_item = np.stack([_frame(k, h, w) for k in kinds for _ in tabs])
    dflt, sse = _plan(frames, _items(tabs * 2), mode, pf, [0, _abi.RUN_SSE], nq=4)
    _equals_ref(dflt, refs, per_item, h, w)
    _equals_ref(sse, refs, per_item, h, w, sse=True)


# ---- 16x16 blocks -------------------------------------------------------------------

@pytest.mark.parametrize('h,w,mode,pf', [(48, 40, '4:2:2', True), (64, 64, '4:2:0', False)])
def test_block16_tables(h, w, mode, pf):
    from jds import _abi
    tabs = ['chroma50', 'flat255', 'one_fine', 'primes']
    kinds = ['random', 'prim', 'half', 'random']
    frames = np.stack([_frame(k, h, w) for k in kinds])
    refs = [_ref(k, h, w, t, mode, pf, None, 16) for k, t in zip(kinds, tabs)]
    runs = _plan(frames, _items(tabs, bs=16), mode, pf, [0, _abi.RUN_EXACT, _abi.RUN_FWD_FIXALL])
    for r in runs:
        _equals_ref(r, refs, frames, h, w, bs=16)
    _agree(runs)
    assert runs[2][3][0] == sum(r['coeffs'].size // 256 for r in refs)  # every block recomputed


# ---- general geometry and the context path ----------------------------------------

@pytest.mark.parametrize('h,w,mode,pf', [(71, 97, '4:2:0', True), (48, 41, '4:2:2', False)])
def test_general_geometry_tables(h, w, mode, pf):
    from jds import _abi
    tabs = ['luma50_T', 'rand_b', 'flat1']
    kinds = ['random', 'prim', 'half']
    frames = np.stack([_frame(k, h, w) for k in kinds])
    refs = [_ref(k, h, w, t, mode, pf, None) for k, t in zip(kinds, tabs)]
    runs = _plan(frames, _items(tabs), mode, pf, [0, _abi.RUN_EXACT, _abi.RUN_SSE])
    for r in runs:
        _equals_ref(r, refs, frames, h, w, sse=r is runs[2])
    _agree(runs)


def _context_equals_ref(img, table, mode, pf, taps):
    from jds import codec
    got = codec.compress_reconstruct_raw(img, 50, table, mode, pf, gauss=taps)
    ref = params_ref.compress_reconstruct(img, table, mode, pf, cpu_ref.gaussian_kernel3(0.75) if taps is None else taps)
    assert np.array_equal(got['coeffs'], ref['coeffs'])
    assert np.array_equal(got['reconstructed'], ref['reconstructed'])
    assert np.array_equal(got['error_map_y'], ref['error_map_y'])
    st = got['stats']
    assert [int(v) for v in st.hist] == [int(v) for v in ref['hist']]
    assert int(st.nonzero) == ref['bitrate']['nonzero_count']
    assert int(st.total_coeffs) == ref['bitrate']['total_coeffs']


@pytest.mark.parametrize('h,w', [(37, 53), (3, 3)])
def test_context_path_on_a_random_table(h, w):
    img = cpu_ref.random_image(h, w, 2400)
    for mode, pf in (('4:2:0', True), ('4:2:2', False), ('4:4:4', False)):
        _context_equals_ref(img, TABLES['rand_a'], mode, pf, None)


# ---- taps ---------------------------------------------------------------------------

TAPS_GEO = [(72, 136, '4:2:0', 8), (32, 136, '4:2:2', 8), (48, 40, '4:2:2', 16), (71, 97, '4:2:0', 8)]


@pytest.mark.parametrize('h,w,mode,bs', TAPS_GEO)
@pytest.mark.parametrize('taps', sorted(TAPS))
def test_prefilter_taps(taps, h, w, mode, bs):
    """Every accepted taps vector, certified against exact, full run against two
    calls: the reference's coefficients and bytes."""
    from jds import _abi
    tabs = ['chroma50', 'flat1']
    kinds = ['random', 'cb_sign', 'cr_sign']
    pairs = [(k, t) for k in kinds for t in tabs]
    frames = np.stack([_frame(k, h, w) for k, _ in pairs])
    refs = [_ref(k, h, w, t, mode, True, taps, bs) for k, t in pairs]
    items = _items([t for _, t in pairs], taps, bs)
    runs = _plan(frames, items, mode, True, [0, _abi.RUN_EXACT, _abi.RUN_INV_FIXALL])
    runs.append(_two_calls(frames, items, mode, True))
    for r in runs:
        _equals_ref(r, refs, frames, h, w, bs=bs)
    _agree(runs)
    general = bool(h % 2 or w % 2)
    if taps in ('sub1', 'over1') and not general:
        # the level shift's 128 |S^2 - 1| exceeds Q / 2: no chroma block is certified
        ph, pw = (h // 2 if mode == '4:2:0' else h), w // 2
        chroma_blocks = len(items) * 2 * -(-ph // bs) * -(-pw // bs)
        print(f'{taps} {h}x{w} {mode} {bs}x{bs}: fix_counts {runs[0][3]}, chroma blocks {chroma_blocks}, '
              f'all blocks {sum(r["coeffs"].size for r in refs) // (bs * bs)}')
        assert runs[0][3][0] >= chroma_blocks
    if taps == 'sharp2':
        # beyond the full run's fixed bound: the plan must track the bound instead (apriori_ok false)
        assert not apriori_ok(TAPS[taps])
        flat1 = [i for i, (_, t) in enumerate(pairs) if t == 'flat1']
        assert np.abs(runs[0][1][flat1].astype(np.int64)).max() > DMAX


@pytest.mark.parametrize('taps', ['gauss2', 'sub1', 'sharp2'])
def test_context_path_and_stage_take_the_taps(taps):
    from jds import codec
    img = cpu_ref.random_image(37, 53, 2401)
    ycc = cpu_ref.rgb_to_ycbcr(img.astype(np.float64))
    for mode in ('4:2:0', '4:2:2'):
        _context_equals_ref(img, TABLES['chroma50'], mode, True, TAPS[taps])
        cb, cr = codec.stage_subsample(ycc[:, :, 1], ycc[:, :, 2], mode, True, gauss=TAPS[taps])
        rcb, rcr = params_ref.subsample(ycc[:, :, 1], ycc[:, :, 2], mode, True, TAPS[taps])
        assert np.array_equal(cb, rcb) and np.array_equal(cr, rcr)
    # None is the reference's Gaussian
    a = codec.compress_reconstruct_raw(img, 50, TABLES['chroma50'], '4:2:0', True)
    b = codec.compress_reconstruct_raw(img, 50, TABLES['chroma50'], '4:2:0', True, gauss=cpu_ref.gaussian_kernel3(0.75))
    assert np.array_equal(a['coeffs'], b['coeffs']) and np.array_equal(a['reconstructed'], b['reconstructed'])


# ---- refusals -----------------------------------------------------------------------

@pytest.mark.parametrize('bad', sorted(BAD_TAPS))
def test_bad_taps_refused_on_the_device_entry_points(bad):
    from jds import _abi, codec
    taps = BAD_TAPS[bad]
    msg = r'prefilter taps \[.*\] must be finite and symmetric'
    h, w = 32, 48
    img = _frame('random', h, w)
    ycc = cpu_ref.rgb_to_ycbcr(img.astype(np.float64))
    Q = TABLES['chroma50']
    for mode in ('4:2:0', '4:2:2'):
        with pytest.raises(ValueError, match=msg):
            _abi.Plan(_abi.context(0), [_abi.make_params(50, Q, mode, True, taps)], h, w)
        with pytest.raises(ValueError, match=msg):
            _abi.Plan(_abi.context(0), [_abi.make_params(50, Q, mode, True, taps, 16)], h, w)
        with pytest.raises(ValueError, match=msg):
            codec.compress_reconstruct_raw(img, 50, Q, mode, True, gauss=taps)
        with pytest.raises(ValueError, match=msg):
            codec.stage_subsample(ycc[:, :, 1], ycc[:, :, 2], mode, True, gauss=taps)
    # the context and a following valid plan still work; without the prefilter the taps stay ignored
    _context_equals_ref(img, Q, '4:2:0', True, None)
    a = codec.compress_reconstruct_raw(img, 50, Q, '4:2:0', False, gauss=taps)
    b = codec.compress_reconstruct_raw(img, 50, Q, '4:2:0', False)
    assert np.array_equal(a['coeffs'], b['coeffs']) and np.array_equal(a['reconstructed'], b['reconstructed'])
    full, = _plan(img[None], [(Q, None, 8)], '4:2:0', True, [0])
    _equals_ref(full, [_ref('random', h, w, 'chroma50', '4:2:0', True, None)], img[None], h, w)
