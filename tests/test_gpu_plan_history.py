"""A jds_plan's run-history state over long sequences of runs on changing frames.

A plan re-arms its device counters for the next run from inside the kernels of
the current one (no memsets): the fast inverse's run counters alternate
(period 2), its per-item counts rotate over three slots, every 16th fast
inverse is a probe run, the 8x8 and 16x16 forwards alternate their counter
banks, and the statistics are reset by the forward's front end.  Here one plan
stays alive for 50+ fast-inverse runs (the lcm of 2, 3 and 16; probes at fast
runs 15, 31 and 47) while every item's content changes from run to run, so that
items enter exact mode, are held there, and are released or kept by a probe.

After every run, bit for bit: coefficients, bytes and statistics equal the CPU
oracle's for that run's content (the bytes may never depend on history);
fix_counts()[1] equals tests/plan_history_model.py fed with each content's
fresh count U (measured on the first run of a fresh one-item plan, per run
kind: a full run certifies a priori, an inverse-only run with the tracked
bound); fix_counts()[0] equals the sum of the fresh forward counts F of this
run's contents alone."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from oracle import cpu_ref
from plan_history_model import PlanHistoryModel
import test_gpu_inv_fast16
import test_gpu_inv_yoff

pytestmark = pytest.mark.gpu

STAT_FIELDS = ('nonzero', 'magnitude_bits', 'hist', 'total_coeffs')
FAST_RUNS = 50  # per sequence: > lcm(2, 3, 16) = 48, three probe runs

# qs: one quality per item (item = frame * nq + q); base: flags of every run
Rig = namedtuple('Rig', 'name h w mode pf bs qs nq base')

RIGS = {r.name: r for r in [
    # 16 tiles of 64 x 128, aligned (inv_yoff == 0): U == 2 pins the '>' of prev * 8 > ntile
    Rig('420', 256, 512, '4:2:0', False, 8, (50, 50, 50, 50), 1, 0),
    # raised tiles (inv_yoff == 8): 2 x 4 tiles of 56 / 64 rows
    Rig('420pf', 120, 512, '4:2:0', True, 8, (50, 50, 50), 1, 0),
    Rig('422', 96, 384, '4:2:2', True, 8, (50, 50, 50), 1, 0),        # 3 x 3 tiles of 32 x 128
    Rig('444', 72, 136, '4:4:4', False, 8, (50, 90, 10), 1, 0),        # 153 blocks: 20 waves of 8
    Rig('sweep', 128, 512, '4:2:0', True, 8, (10, 50, 95) * 2, 3, 0),  # Q10 items start seeded
    Rig('mixed', 128, 512, '4:2:0', False, 8, (10, 50, 10, 50), 1, 0),
    Rig('coarse', 96, 384, '4:2:2', False, 8, (10, 5, 10), 1, 128),    # RUN_INV_FAST on every run
    Rig('b16', 96, 384, '4:2:2', False, 16, (50, 90, 20), 1, 0),       # k_inv16_fast, Fwd16Fast
]}


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


def _table(q):
    return cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, q)


def _coarse(q):
    return float(np.asarray(_table(q)).reshape(-1)[0]) > 60.0


def _adaptive(rig):
    return rig.bs == 8 and rig.mode != '4:4:4'


def _seeded(rig):
    """jds_plan_create_q: mixed 8x8 4:2:x plans seed their coarse items."""
    if not _adaptive(rig):
        return [False] * len(rig.qs)
    c = [_coarse(q) for q in rig.qs]
    return [x and not all(c) for x in c]


def _tiles(rig):
    """Units of fix_counts()[1] per item: inverse tiles (4:4:4: waves of 8 blocks,
    whole workgroups of 4)."""
    if rig.bs == 16:
        return test_gpu_inv_fast16._tiles(rig.mode, rig.h, rig.w)
    if rig.mode == '4:2:0':
        return test_gpu_inv_yoff._tiles(rig.h, rig.w)
    if rig.mode == '4:2:2':
        return -(-rig.h // 32) * -(-rig.w // 128)
    return 4 * -(-(-(-rig.h // 8) * -(-rig.w // 8)) // 32)


def _gray_tiles(rig, img, k):
    """Gray-128 laid exactly over the first k inverse tiles (raster order)."""
    img = img.copy()
    if rig.mode == '4:4:4':  # wave t: blocks [8 t, 8 t + 8) of the raster block grid
        nbx = -(-rig.w // 8)
        for b in range(8 * k):
            by, bx = divmod(b, nbx)
            img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 128
        return img
    th, tw = (64, 64) if rig.bs == 16 and rig.mode == '4:2:0' else (64, 128) if rig.mode == '4:2:0' else (32, 128)
    yoff = 8 if rig.bs == 8 and rig.mode == '4:2:0' and (rig.h + 8 + 63) // 64 == (rig.h + 63) // 64 else 0
    ntx = -(-rig.w // tw)
    for t in range(k):
        ty, tx = divmod(t, ntx)
        img[max(0, th * ty - yoff):th * ty - yoff + th, tw * tx:tw * tx + tw] = 128
    return img


@functools.lru_cache(maxsize=None)
def _pool(name):
    """The rig's frames: two random ones, flat gray, and a random one with gray
    over 1, nt // 8 and nt // 8 + 1 whole tiles."""
    rig = RIGS[name]
    seed = 7000 + 10 * sorted(RIGS).index(name)
    a = cpu_ref.random_image(rig.h, rig.w, seed)
    nt = _tiles(rig)
    pool = {'rndA': a, 'rndB': cpu_ref.random_image(rig.h, rig.w, seed + 1),
            'gray': np.full((rig.h, rig.w, 3), 128, np.uint8),
            'g1': _gray_tiles(rig, a, 1), 'gb': _gray_tiles(rig, a, nt // 8 + 1)}
    if nt // 8 > 1:
        pool['gs'] = _gray_tiles(rig, a, nt // 8)
    return pool


def _magnitude_bits(coeffs):
    """sum over q != 0 of ceil(log2(|q| + 1)) + 1, in integers."""
    a = np.abs(coeffs.astype(np.int64).reshape(-1))
    a = a[a != 0]
    return int(sum(int(v).bit_length() + 1 for v in a))


class _Live:
    """One plan and `slots` sets of result buffers (a run writes one set)."""

    def __init__(self, rig, qs, nq=1, slots=1):
        import torch
        from jds import _abi, codec
        params = [_abi.make_params(q, _table(q), rig.mode, rig.pf, codec.gaussian_kernel3(), block_size=rig.bs)
                  for q in qs]
        self.plan = _abi.Plan(_abi.context(0), params, rig.h, rig.w, nq=nq)
        self.n, self.nf, self.cpf = len(qs), len(qs) // nq, int(self.plan.geometry.coeffs_per_frame)
        dev = torch.device('cuda:0')
        self.out = torch.zeros((slots, self.n, rig.h, rig.w, 3), dtype=torch.uint8, device=dev)
        self.cf = torch.zeros((slots, self.n, self.cpf), dtype=torch.int16, device=dev)
        self.st = torch.zeros((slots, self.n, _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)

    def run(self, flags, rgb, slot=0, stream=None):
        import torch
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.plan.run(rgb.data_ptr(), self.out[slot].data_ptr(), self.cf[slot].data_ptr(), self.st[slot].data_ptr(),
                      flags, s)

    def stats(self, slot=0):
        from jds import _abi
        return self.st[slot].cpu().numpy().view(_abi.STATS_DTYPE).reshape(-1)

    def close(self):
        self.plan.close()


def _fresh_counts(rig, q, frame, coeffs=None):
    """(U of a full run, U of an inverse-only run, F, magnitude_bits of the exact
    run) of one item, each from the first run of a fresh one-item plan.  With
    `coeffs` (caller-supplied) only the inverse-only U and the exact bytes."""
    import torch
    from jds import _abi
    A = _abi
    rgb = torch.from_numpy(np.ascontiguousarray(frame[None])).cuda()
    fast = rig.base | A.RUN_INV_FAST  # (a coarse one-item plan would pick k_inv2)
    res = {}
    live = _Live(rig, [q])
    if coeffs is None:
        live.run(fast, rgb)
        torch.cuda.synchronize()
        res['F'], res['U_full'] = (int(v) for v in live.plan.fix_counts())
        live.close()
        live = _Live(rig, [q])
        live.run(A.RUN_FWD, rgb)
    else:
        live.cf[0, 0].copy_(torch.from_numpy(coeffs).cuda())
    live.run(fast | A.RUN_INV, rgb)
    torch.cuda.synchronize()
    res['U_inv'] = int(live.plan.fix_counts()[1])
    live.close()
    live = _Live(rig, [q])
    if coeffs is None:
        live.run(A.RUN_EXACT, rgb)
        torch.cuda.synchronize()
        res['magnitude_bits'] = int(live.stats()['magnitude_bits'][0])
    else:
        live.cf[0, 0].copy_(torch.from_numpy(coeffs).cuda())
        live.run(A.RUN_INV | A.RUN_EXACT_INV, rgb)
        torch.cuda.synchronize()
        res['reconstructed'] = live.out[0, 0].cpu().numpy()
    live.close()
    return res


@functools.lru_cache(maxsize=None)
def _expect(name):
    """Per (content, quality) of the rig: the oracle's results and the fresh
    counts; 'nt' from a fresh fix-all run; for sweep plans F per content from a
    fresh one-frame sweep plan (their forward is another kernel chain)."""
    import torch
    from jds import _abi
    rig, pool = RIGS[name], _pool(name)
    E = {}
    for q in sorted(set(rig.qs)):
        for c, frame in pool.items():
            ref = cpu_ref.compress_reconstruct(frame, q, rig.bs, rig.mode, rig.pf, metrics=False,
                                               stretch=rig.bs == 16)
            e = {'coeffs': np.ascontiguousarray(ref['coeffs']).reshape(-1).astype(np.int16),
                 'reconstructed': np.ascontiguousarray(ref['reconstructed']),
                 'hist': np.asarray(ref['hist']).astype(np.uint64),
                 'nonzero': int(ref['bitrate']['nonzero_count']),
                 'sse_rgb': int(((frame.astype(np.int64) - ref['reconstructed']) ** 2).sum())}
            e.update(_fresh_counts(rig, q, frame))
            assert e['magnitude_bits'] == _magnitude_bits(e['coeffs']), (name, c, q)
            e['total_coeffs'] = e['coeffs'].size
            E[c, q] = e
    live = _Live(rig, rig.qs, rig.nq)
    rgb = torch.from_numpy(np.stack([pool['rndA']] * live.nf)).cuda()
    live.run(rig.base | _abi.RUN_INV_FIXALL, rgb)
    torch.cuda.synchronize()
    total = int(live.plan.fix_counts()[1])
    live.close()
    assert total % live.n == 0 and total // live.n == _tiles(rig), (name, total, _tiles(rig))
    E['nt'] = total // live.n
    if rig.nq > 1:
        for c, frame in pool.items():
            live = _Live(rig, rig.qs[:rig.nq], rig.nq)
            live.run(0, torch.from_numpy(np.ascontiguousarray(frame[None])).cuda())
            torch.cuda.synchronize()
            E['F', c] = int(live.plan.fix_counts()[0])
            live.close()
    return E


def _classes(name, kind='U_full'):
    """Which of the four classes of U the rig's (content, quality) pairs fall in."""
    E = _expect(name)
    nt, out = E['nt'], {}
    for key, e in E.items():
        if isinstance(key, tuple) and key[0] != 'F':
            u = e[kind]
            cls = 'zero' if u == 0 else 'small' if u * 8 <= nt else 'big' if u < nt else 'all'
            out.setdefault(cls, []).append((key, u))
    return out


# ------------------------------------------------------------- schedules --

def _flags(kind):
    from jds import _abi as A
    return {'full': 0, 'sse': A.RUN_SSE, 'fixall': A.RUN_INV_FIXALL, 'exact': A.RUN_EXACT | A.RUN_SSE,
            'exact_inv': A.RUN_EXACT_INV, 'fwd': A.RUN_FWD, 'inv': A.RUN_INV, 'inv_sse': A.RUN_INV | A.RUN_SSE,
            'fwd_fixall': A.RUN_FWD_FIXALL}[kind]


PATTERN8 = ('full', 'sse', 'inv', 'full', 'exact_inv', 'full', 'fwd', 'inv_sse', 'full', 'exact', 'sse', 'full', 'inv')
PATTERN16 = ('full', 'inv', 'fwd_fixall', 'full', 'exact_inv', 'fwd', 'full', 'exact', 'sse', 'fwd_fixall', 'inv',
             'full', 'fwd')
FIXALL_AT = 36  # the fast run that is a RUN_INV_FIXALL run; plain runs follow it


def _content(k, f, names, rng):
    """Content of frame f while `k` fast inverses have run.  Frame 0: flat at
    run 0 (enters exact mode), random while held there, flat again at the probe
    (run 15: stays), random at the next probe (run 31: leaves), a many-tile
    content at run 33 (enters again), a one-tile content at the probe of run 47
    (leaves).  Frame 1: random / few-tile contents through the first probe (not
    in exact mode), flat at run 20 (enters, opposite to frame 0 before), flat at
    the probe of run 31 (stays), random at the probe of run 47.  Others: seeded
    random picks."""
    small = 'gs' if 'gs' in names else 'g1'
    if f == 0:
        if k in (0, 15):
            return 'gray'
        if k == 33:
            return 'gb'
        if k == 47:
            return 'g1'
        return ('rndA', 'rndB', 'g1')[k % 3] if k < 31 else ('rndA', 'rndB')[k % 2]
    if f == 1:
        if k in (20, 31):
            return 'gray'
        if k == 47:
            return 'rndB'
        return ('rndB', 'g1', 'rndA', small)[k % 4] if k < 20 else ('rndB', 'rndA')[k % 2]
    return names[int(rng.integers(len(names)))]


def _model_kind(rig, flags):
    from jds import _abi as A
    if (flags & A.RUN_FWD) and not (flags & A.RUN_INV):
        return 'fwd_only'
    fast = not (flags & (A.RUN_EXACT | A.RUN_EXACT_INV))
    if rig.bs == 8 and rig.mode != '4:4:4' and all(_coarse(q) for q in rig.qs):
        fast = fast and bool(flags & A.RUN_INV_FAST)  # all-coarse 4:2:x plans run k_inv2 unless asked
    if (flags & A.RUN_SSE) and (rig.bs == 16 or rig.mode == '4:4:4'):
        fast = False  # SSE runs of these take the exact kernels
    if not fast:
        return 'exact_inv'
    return 'fast_fixall' if flags & A.RUN_INV_FIXALL else 'fast'


def _schedule(name, seed):
    """[(flags, contents per frame, model Step, expected fix_counts()[0] or None)]
    until FAST_RUNS fast inverses have run (the model is stepped along)."""
    from jds import _abi as A
    rig, E = RIGS[name], _expect(name)
    names = sorted(_pool(name))
    n, nf = len(rig.qs), len(rig.qs) // rig.nq
    model = PlanHistoryModel(n, E['nt'], adaptive=_adaptive(rig), seeded=_seeded(rig))
    rng = np.random.default_rng(seed)
    pattern = PATTERN16 if rig.bs == 16 else PATTERN8
    sched, t, fixall_done, fwd_count = [], 0, False, 0
    while model.inv_runs < FAST_RUNS:
        kind = pattern[t % len(pattern)]
        t += 1
        if model.inv_runs == FIXALL_AT and not fixall_done:
            kind, fixall_done = 'fixall', True
        flags = _flags(kind) | rig.base
        cs = [_content(model.inv_runs, f, names, rng) for f in range(nf)]
        item_c = [cs[i // rig.nq] for i in range(n)]
        full = not (flags & (A.RUN_FWD | A.RUN_INV))
        step = model.step(_model_kind(rig, flags),
                          [E[item_c[i], rig.qs[i]]['U_full' if full else 'U_inv'] for i in range(n)])
        if not (flags & A.RUN_INV) or (flags & A.RUN_FWD):  # the forward runs
            if flags & A.RUN_EXACT:
                fwd_count = 0 if rig.bs == 16 else None  # 8x8: not pinned after an exact forward
            elif flags & A.RUN_FWD_FIXALL:
                fwd_count = n * (E[item_c[0], rig.qs[0]]['coeffs'].size // 256)
            elif rig.nq > 1:
                fwd_count = sum(E['F', c] for c in cs)
            else:
                fwd_count = sum(E[item_c[i], rig.qs[i]]['F'] for i in range(n))
        sched.append((flags, cs, step, fwd_count))
    return sched


# ---------------------------------------------------------------- driver --

def _drive(name, seed, stream_order=False):
    """Generator: runs the rig's schedule on one plan, one run per next().  With
    stream_order: no synchronisation and no fix_counts() between the runs, every
    run into its own slot, everything compared after the last one."""
    import torch
    from jds import _abi as A
    rig, E, pool = RIGS[name], _expect(name), _pool(name)
    names = sorted(pool)
    sched = _schedule(name, seed)
    n = len(rig.qs)
    bad = []
    stream = torch.cuda.Stream() if stream_order else torch.cuda.current_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        live = _Live(rig, rig.qs, rig.nq, slots=len(sched) if stream_order else 1)
        pool_dev = torch.from_numpy(np.stack([pool[c] for c in names])).cuda()
        keys = sorted({(c, q) for c in names for q in set(rig.qs)})
        want_cf = {k: torch.from_numpy(E[k]['coeffs']).cuda() for k in keys}
        want_out = {k: torch.from_numpy(E[k]['reconstructed']).cuda() for k in keys}

        def items(cs):
            return [(cs[i // rig.nq], rig.qs[i]) for i in range(n)]

        def prepare(slot, flags, cs):
            # nothing a run should write may already hold the right values; the
            # statistics start as garbage (the forward's front end resets them)
            if flags & A.RUN_INV and not flags & A.RUN_FWD:
                for i, k in enumerate(items(cs)):
                    live.cf[slot, i].copy_(want_cf[k])
                live.st[slot].zero_()
            else:
                live.cf[slot].zero_()
                live.st[slot].fill_(0xA5)
            live.out[slot].zero_()

        def check(r, slot, flags, cs, stats):
            fwd = not (flags & A.RUN_INV) or bool(flags & A.RUN_FWD)
            inv = not (flags & A.RUN_FWD) or bool(flags & A.RUN_INV)
            for i, k in enumerate(items(cs)):
                e = E[k]
                if not torch.equal(live.cf[slot, i], want_cf[k]):
                    bad.append((r, flags, i, k, 'coeffs'))
                if inv and not torch.equal(live.out[slot, i], want_out[k]):
                    bad.append((r, flags, i, k, 'rgb_out', int((live.out[slot, i] != want_out[k]).sum())))
                if fwd:
                    for f in STAT_FIELDS:
                        if not np.array_equal(stats[i][f], e[f]):
                            bad.append((r, flags, i, k, f, stats[i][f].tolist(), np.asarray(e[f]).tolist()))
                if inv and flags & A.RUN_SSE and int(stats[i]['sse_rgb']) != e['sse_rgb']:
                    bad.append((r, flags, i, k, 'sse_rgb', int(stats[i]['sse_rgb']), e['sse_rgb']))

        def counts(r, flags, step, fwd_count):
            fix = live.plan.fix_counts()
            if int(fix[1]) != step.count:
                bad.append((r, flags, 'fix_counts[1]', int(fix[1]), step))
            if fwd_count is not None and int(fix[0]) != fwd_count:
                bad.append((r, flags, 'fix_counts[0]', int(fix[0]), fwd_count))

        try:
            if stream_order:
                idx = torch.tensor([[names.index(c) for c in cs] for _, cs, _, _ in sched], device='cuda')
                rgb_all = pool_dev[idx]  # [R, frames, H, W, 3]
                for r, (flags, cs, _, _) in enumerate(sched):
                    prepare(r, flags, cs)
                for r, (flags, cs, _, _) in enumerate(sched):
                    live.run(flags, rgb_all[r], slot=r, stream=stream.cuda_stream)
                    yield r
                torch.cuda.synchronize()
                for r, (flags, cs, _, _) in enumerate(sched):
                    check(r, r, flags, cs, live.stats(r))
                counts(len(sched) - 1, *sched[-1][::2], sched[-1][3])
            else:
                for r, (flags, cs, step, fwd_count) in enumerate(sched):
                    prepare(0, flags, cs)
                    rgb = pool_dev[torch.tensor([names.index(c) for c in cs], device='cuda')]
                    live.run(flags, rgb)
                    torch.cuda.synchronize()
                    check(r, 0, flags, cs, live.stats(0))
                    counts(r, flags, step, fwd_count)
                    yield r
        finally:
            live.close()
    assert not bad, (name, len(bad), bad[:8])


def _run_all(gen):
    for _ in gen:
        pass


def _trace(name, seed):
    """The fast runs of the schedule: (Step, U per item as this run's contents measure)."""
    from jds import _abi as A
    rig, E = RIGS[name], _expect(name)
    out = []
    for flags, cs, step, _ in _schedule(name, seed):
        if step.kind in ('fast', 'fast_fixall'):
            full = not (flags & (A.RUN_FWD | A.RUN_INV))
            out.append((step, [E[cs[i // rig.nq], rig.qs[i]]['U_full' if full else 'U_inv']
                               for i in range(len(rig.qs))]))
    return out


# ----------------------------------------------------------------- tests --

@pytest.mark.parametrize('name', ['420', '420pf', '422'])
def test_adaptive_single_quality_sequences(name):
    """All four classes of U are in the pool as measured, the schedule takes
    every branch of the exact-mode machine (read off the model's trace), and the
    plan matches the oracle and the model on every run."""
    E = _expect(name)
    nt = E['nt']
    for kind in ('U_full', 'U_inv'):
        cls = _classes(name, kind)
        assert set(cls) == {'zero', 'small', 'big', 'all'}, (name, kind, cls)
    if name == '420':
        assert nt == 16 and RIGS[name].h % 64 == 0
        assert any(u * 8 == nt for _, u in _classes(name)['small']), _classes(name)  # pins '>'
    tr = _trace(name, 1)
    assert len(tr) >= FAST_RUNS and [s.probe for s, _ in tr].count(True) == 3
    held = lambda s, i: s.prev[i] * 8 > nt  # noqa: E731  (in exact mode but for a probe / fix-all)
    # an item enters exact mode and gets random content while there
    assert any(s.exact[i] and u[i] == 0 for s, u in tr for i in range(len(u)))
    # a probe finds an item in exact mode: with flat content it stays, with random content it leaves
    nxt = {id(s): tr[j + 1][0] for j, (s, _) in enumerate(tr[:-1])}
    probes = [(s, u) for s, u in tr if s.probe]
    assert any(held(s, i) and u[i] == nt and nxt[id(s)].exact[i] for s, u in probes for i in range(len(u)))
    assert any(held(s, i) and u[i] * 8 <= nt and not nxt[id(s)].exact[i] for s, u in probes for i in range(len(u)))
    assert any(not held(s, i) for s, u in probes for i in range(len(u)))
    # two items in opposite modes in one run; a fix-all run with plain runs after it
    assert any(True in s.exact and False in s.exact for s, _ in tr)
    fa = [j for j, (s, _) in enumerate(tr) if s.kind == 'fast_fixall']
    assert fa == [FIXALL_AT] and all(tr[FIXALL_AT + 1][0].exact)
    kinds = {s.kind for _, _, s, _ in _schedule(name, 1)}
    assert kinds == {'fast', 'fast_fixall', 'exact_inv', 'fwd_only'}
    _run_all(_drive(name, 1))


def test_444_sequence_wave_local_kernel():
    """k_inv_fast444 / k_fwd444w: the counters alternate and rotate, no exact
    mode.  RUN_SSE runs at 4:4:4 take the exact inverse: they count as
    exact-inverse runs (fix_counts()[1] == 0) and the next fast run counts from
    zero."""
    assert not _adaptive(RIGS['444'])
    assert {'zero', 'all'} <= set(_classes('444'))
    _run_all(_drive('444', 2))


@pytest.mark.parametrize('seed', [3, 4])
def test_sweep_plan_sequences(seed):
    """nq = 3 at (10, 50, 95) on two frames, RUN_SSE runs among the plain ones
    (k_inv_fast's XTRA = 1 instantiations).  The Q10 items start seeded into
    exact mode: their first fast measurement is the first probe run."""
    rig = RIGS['sweep']
    seeded = _seeded(rig)
    assert seeded == [True, False, False] * 2
    tr = _trace('sweep', seed)
    for i, s in enumerate(seeded):
        first = next(j for j, (st, _) in enumerate(tr) if not st.exact[i])
        assert first == (15 if s else 0), (i, first)
    _run_all(_drive('sweep', seed))


def test_mixed_single_quality_plan_sequence():
    """Q10 and Q50 items of one jds_plan_create: the coarse ones seeded."""
    assert _seeded(RIGS['mixed']) == [True, False, True, False]
    tr = _trace('mixed', 5)
    assert all(st.exact[0] and st.exact[2] for st, _ in tr[:15]) and not any(tr[15][0].exact)
    _run_all(_drive('mixed', 5))


def test_all_coarse_plan_driven_fast():
    """Every table coarse: nothing is seeded, the plan's own route is k_inv2 and
    RUN_INV_FAST on every run drives the certified kernel through its cycles."""
    assert _seeded(RIGS['coarse']) == [False] * 3
    _run_all(_drive('coarse', 6))


def test_b16_sequence_inverse_and_forward_parity():
    """16x16 4:2:2: k_inv16_fast (no exact mode) and the certified forward's
    alternating list counters (Fwd16Fast::parity), RUN_FWD_FIXALL runs between."""
    sched = _schedule('b16', 7)
    from jds import _abi as A
    assert sum(1 for fl, *_ in sched if fl & A.RUN_FWD_FIXALL) >= 5
    assert all(c is not None for *_, c in sched)
    _run_all(_drive('b16', 7))


@pytest.mark.parametrize('name,seed', [('420', 1), ('sweep', 3)])
def test_stream_order_without_host_syncs(name, seed):
    """The same sequences on a non-default stream, no synchronisation and no
    fix_counts() between the runs: the kernels' stream order alone re-arms the
    counters.  Every run's slot is compared after one final synchronisation."""
    _run_all(_drive(name, seed, stream_order=True))


def test_two_plans_interleaved_on_one_context():
    """Two plans of different shape alternate runs on one context, each on its
    own schedule: neither's history leaks into the other's."""
    a, b = _drive('420pf', 8), _drive('422', 9)
    done_a = done_b = False
    while not (done_a and done_b):
        if not done_a:
            done_a = next(a, None) is None
        if not done_b:
            done_b = next(b, None) is None


def test_inverse_only_caller_coefficients_change_between_runs():
    """RUN_INV runs whose coefficients are the caller's: arbitrary int16 values
    (scale 32767), then codec output, then arbitrary ones again, per item on a
    shifted rhythm.  Bytes equal a fresh plan's RUN_EXACT_INV bytes on every run;
    the count follows the model (the Q5 item of this mixed plan starts seeded)."""
    import torch
    from jds import _abi as A
    rig = Rig('invonly', 128, 512, '4:2:0', False, 8, (5, 50, 100), 1, 0)
    n = len(rig.qs)
    frames = np.stack([cpu_ref.random_image(rig.h, rig.w, 900 + i) for i in range(n)])
    live = _Live(rig, rig.qs)
    rng = np.random.default_rng(32767)
    arb = np.clip(rng.normal(0, 32767, (n, live.cpf)), -32768, 32767).astype(np.int16)
    codec = np.stack([cpu_ref.compress_reconstruct(frames[i], q, 8, rig.mode, rig.pf, metrics=False)['coeffs']
                      .reshape(-1).astype(np.int16) for i, q in enumerate(rig.qs)])
    src = {'arb': arb, 'codec': codec}
    fresh = {(k, i): _fresh_counts(rig, rig.qs[i], frames[i], coeffs=src[k][i]) for k in src for i in range(n)}
    nt = test_gpu_inv_yoff._tiles(rig.h, rig.w)
    model = PlanHistoryModel(n, nt, seeded=_seeded(rig))
    assert _seeded(rig) == [True, False, False]
    rgb = torch.from_numpy(frames).cuda()
    dev = {(k, i): torch.from_numpy(src[k][i]).cuda() for k in src for i in range(n)}
    want = {k: torch.from_numpy(v['reconstructed']).cuda() for k, v in fresh.items()}
    bad = []
    try:
        for r in range(FAST_RUNS + 2):
            pick = [('arb', 'codec')[((r + 2 * i) // 6) % 2] for i in range(n)]
            for i in range(n):
                live.cf[0, i].copy_(dev[pick[i], i])
            live.out[0].zero_()
            live.run(A.RUN_INV, rgb)
            torch.cuda.synchronize()
            step = model.step('fast', [fresh[pick[i], i]['U_inv'] for i in range(n)])
            for i in range(n):
                if not torch.equal(live.out[0, i], want[pick[i], i]):
                    bad.append((r, i, pick[i], 'rgb_out'))
                if not torch.equal(live.cf[0, i], dev[pick[i], i]):
                    bad.append((r, i, pick[i], 'coeffs changed'))
            if int(live.plan.fix_counts()[1]) != step.count:
                bad.append((r, 'fix_counts[1]', int(live.plan.fix_counts()[1]), step))
    finally:
        live.close()
    assert not bad, (len(bad), bad[:8])
    us = {k: v['U_inv'] for k, v in fresh.items()}
    assert {u * 8 > nt for u in us.values()} == {True, False}, us  # both modes occur
