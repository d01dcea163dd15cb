"""bench.py --dump-outputs / --full.

CPU: dump_outputs writes float32 / float64 arrays, whole when small and a
seeded sample at pinned positions when large (divided among the ranks), and
leaves out the host-path timing fields of the statistics.  GPU: small runs of
bench.py itself -- a plain line carries the headline fields only and dumps the
last timed step's outputs; --full adds the other legs and dumps the same
arrays; with --pipeline 1 the dump is the buffer set of the last timed step;
the sweep path dumps every item."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from jds import _abi  # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup')
FULL_ONLY = ('roofline', 'kernels_ms', 'kernels_profile', 'fixups_last_step', 'entropy', 'parity', 'host_path')
SWEEP_FULL_ONLY = ('gather', 'ssim', 'parity')
NAMES = (('reconstructed', np.float32), ('coefficients', np.float32), ('stats', np.float64))
F, H, W = 3, 80, 112
SMALL = ['--warmup', '1', '--frames', str(F), '--height', str(H), '--width', str(W)]


def _stats(n):
    st = np.zeros(n, dtype=_abi.STATS_DTYPE)
    st['nonzero'] = np.arange(n) + 7
    st['hist'][:, 3] = 5
    st['sse_y'] = 0.5
    st['fwd_ms'] = 123.0  # host-path timing: never dumped
    return torch.from_numpy(st.view(np.uint8).reshape(n, -1).copy())


def test_dump_small_arrays_whole(tmp_path):
    out = torch.arange(2 * 4 * 6 * 3, dtype=torch.int64).reshape(2, 4, 6, 3).to(torch.uint8)
    cf = (torch.arange(2 * 40, dtype=torch.int32).reshape(2, 40) - 40).to(torch.int16)
    bench.dump_outputs(str(tmp_path), out, cf, _stats(2))
    rec, co, st = (np.load(tmp_path / f'{n}.npy') for n in ('reconstructed', 'coefficients', 'stats'))
    assert rec.dtype == np.float32 and np.array_equal(rec, out.numpy().reshape(-1))
    assert co.dtype == np.float32 and np.array_equal(co, cf.numpy().reshape(-1))
    names = [f for f in _abi.STATS_DTYPE.names if f not in bench.DUMP_STATS_SKIP]
    width = sum(int(np.prod(_abi.STATS_DTYPE[f].shape, dtype=np.int64)) for f in names)
    assert st.dtype == np.float64 and st.shape == (2, width)
    assert st[:, 0].tolist() == [7.0, 8.0] and 123.0 not in st
    assert st[0, 4 + 3] == 5.0  # hist follows the four leading counters, flattened in place


def test_dump_large_array_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    out = (torch.arange(5000, dtype=torch.int64) % 251).to(torch.uint8)
    cf = torch.zeros(10, dtype=torch.int16)
    a, b = tmp_path / 'a', tmp_path / 'b'
    bench.dump_outputs(str(a), out, cf, _stats(1))
    bench.dump_outputs(str(b), out, cf, _stats(1), rank=1)
    x, y = np.load(a / 'reconstructed.npy'), np.load(b / 'reconstructed.rank1.npy')
    assert x.shape == (1000,) and x.dtype == np.float32 and np.array_equal(x, y)
    # the positions are part of the format (two builds are compared file against file): seed
    # 20240229, torch.randint on the CPU generator, sorted -- pinned here for 1000 of 5000
    idx = _sample_positions(5000, 1000)
    assert idx[:8].tolist() == [2, 3, 5, 6, 9, 14, 20, 24] and idx[-4:].tolist() == [4965, 4970, 4978, 4978]
    src = out.numpy().astype(np.float32)
    assert np.array_equal(x, src[idx])
    # N ranks share the sample: each keeps DUMP_SAMPLE // N positions
    c = tmp_path / 'c'
    bench.dump_outputs(str(c), out, cf, _stats(1), rank=0, world=4)
    z = np.load(c / 'reconstructed.npy')
    assert z.shape == (250,) and np.array_equal(z, src[_sample_positions(5000, 250)])


def _sample_positions(n, k):
    g = torch.Generator()
    g.manual_seed(20240229)
    idx = torch.randint(0, n, (k,), generator=g).sort().values.numpy()
    if (n, k) == (5000, 1000):
        assert int(idx.sum()) == 2526853  # the pinned draw
    return idx


def _run(args, timeout=170):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + args,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return lines[0]


def _load(d):
    return {n: np.load(os.path.join(d, n + '.npy')) for n, _ in NAMES}


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('plain'))
    return _run(SMALL + ['--steps', '3', '--dump-outputs', d]), _load(d)


@pytest.mark.gpu
def test_plain_line_is_the_headline_only(plain):
    line, dump = plain
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY + ('north_star',))
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'Mpixels/s' and line['higher_is_better']
    # ms_per_step is printed to 1e-4 ms and a step of this size takes more than 0.01 ms
    assert line['ms_per_step'] > 0.01
    assert line['value'] == pytest.approx(F * H * W / (line['ms_per_step'] * 1e-3) / 1e6, rel=1e-2)
    for n, dt in NAMES:
        assert dump[n].dtype == dt
    cpf = H * W + 2 * (H // 2) * (W // 2)  # 4:2:0, every plane a whole number of 8x8 blocks
    assert dump['reconstructed'].shape == (F * H * W * 3,) and dump['coefficients'].shape == (F * cpf,)
    assert dump['stats'].shape[0] == F and dump['reconstructed'].max() <= 255 and dump['reconstructed'].min() >= 0
    assert np.array_equal(dump['stats'][:, 1], np.full(F, cpf, dtype=np.float64))  # total_coeffs


@pytest.mark.gpu
def test_full_line_adds_the_other_legs_and_dumps_the_same(plain, tmp_path):
    line, dump = plain
    full = _run(SMALL + ['--steps', '3', '--full', '--no-cpu-baseline', '--dump-outputs', str(tmp_path)])
    assert all(k in full for k in HEADLINE + FULL_ONLY)
    assert full['parity']['coeff_mismatch'] == 0 and full['parity']['recon_mismatch_bytes'] == 0
    assert full['kernels_profile']['profiled_step_ms'] > 0 and full['roofline']['kernel'] in full['kernels_ms']
    for k in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps'):
        assert line[k] == full[k]
    got = _load(str(tmp_path))
    for n, _ in NAMES:
        assert np.array_equal(dump[n], got[n]), n


@pytest.mark.gpu
def test_pipeline_dump_is_the_last_steps_buffer_set(plain, tmp_path):
    """Two buffer sets, the timed steps start on set 0: 3 steps end on set 0,
    whose frames are the generator's first draw -- the frames of the plain run --
    and 2 steps end on set 1, other frames."""
    _, dump = plain
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    _run(SMALL + ['--pipeline', '1', '--steps', '3', '--dump-outputs', a])
    _run(SMALL + ['--pipeline', '1', '--steps', '2', '--dump-outputs', b])
    s0, s1 = _load(a), _load(b)
    for n in ('reconstructed', 'coefficients'):
        assert np.array_equal(s0[n], dump[n]), n
        assert s1[n].shape == dump[n].shape and not np.array_equal(s1[n], dump[n]), n


@pytest.mark.gpu
def test_sweep_dump_holds_every_item(tmp_path):
    line = _run(['--sweep', '--steps', '2', '--warmup', '1', '--frames', '2', '--height', str(H), '--width', str(W),
                 '--dump-outputs', str(tmp_path)])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in SWEEP_FULL_ONLY)
    assert line['steps'] == 2
    nq = len(bench.SWEEP_QS)
    d = _load(str(tmp_path))
    cpf = H * W + 2 * (H // 2) * (W // 2)
    assert d['reconstructed'].shape == (2 * nq * H * W * 3,) and d['coefficients'].shape == (2 * nq * cpf,)
    assert d['stats'].shape[0] == 2 * nq and d['stats'].dtype == np.float64
    # coarser tables leave fewer nonzero coefficients: Q5 < Q50 < Q95 on each frame (column 0 = nonzero)
    nz = d['stats'][:, 0].reshape(2, nq)
    assert np.all(nz[:, 0] < nz[:, 3]) and np.all(nz[:, 3] < nz[:, 5])
