"""Re-entrancy of the drop-in boundary.

The reference's callers run compress_reconstruct from Qt worker threads, and
dialogs can run concurrently with the main tab (gui/worker.py:10-36,
gui/dialogs/aliasing_demo_dialog.py:158, gui/dialogs/report_exporter.py:107).
Here two Python threads call the drop-in at the same time (ctypes releases the
GIL, so the two C-ABI calls overlap on the device) on different sizes and
modes, and every result must be bit-exact with the oracle.  Short-lived
threads must reuse pooled contexts (jds._abi.lease) rather than create a HIP
stream and scratch per run."""
import threading

import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import _abi
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


JOBS = [
    [(cpu_ref.random_image(270, 480, 41), 50, '4:2:0', True), (cpu_ref.random_image(37, 53, 42), 30, '4:2:0', False),
     (cpu_ref.random_image(128, 96, 43), 90, '4:4:4', False)],
    [(cpu_ref.random_image(200, 333, 44), 75, '4:2:2', True), (cpu_ref.random_image(64, 64, 45), 10, '4:2:0', True),
     (cpu_ref.random_image(81, 160, 46), 50, '4:2:2', False)],
]


def _run(img, q, mode, pf):
    from engines import compress_reconstruct
    from models import CompressionParams
    res, inter = compress_reconstruct(img, CompressionParams(quality=q, subsampling_mode=mode, use_prefilter=pf))
    return res.reconstructed_image, inter.all_quantized_coeffs, res.psnr_y, inter.error_map_rgb


def test_two_threads_concurrent_drop_in_bit_exact():
    refs = [[cpu_ref.compress_reconstruct(img, q, 8, mode, pf) for img, q, mode, pf in jobs] for jobs in JOBS]
    reps = 3
    results = [[None] * (len(JOBS[0]) * reps) for _ in JOBS]
    errors = []
    start = threading.Barrier(len(JOBS))

    def worker(t):
        try:
            start.wait()
            for r in range(reps):
                for j, job in enumerate(JOBS[t]):
                    results[t][r * len(JOBS[t]) + j] = _run(*job)
        except Exception as e:  # surfaced in the main thread
            errors.append(e)

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(len(JOBS))]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths), 'a worker thread hung'
    assert not errors, errors
    for t, jobs in enumerate(JOBS):
        for k, (rec, cf, psnr_y, emap) in enumerate(results[t]):
            ref = refs[t][k % len(jobs)]
            assert np.array_equal(cf, ref['coeffs']), (t, k)
            assert np.array_equal(rec, ref['reconstructed']), (t, k)
            assert np.array_equal(emap, ref['error_map_rgb']), (t, k)
            assert psnr_y == ref['metrics']['psnr_y'], (t, k)


def test_short_lived_threads_reuse_pooled_contexts():
    from jds import _abi
    created = []
    orig = _abi.Context.__init__

    def counting_init(self, device=0):
        created.append(device)
        orig(self, device)

    img = cpu_ref.random_image(40, 56, 47)
    _run(img, 50, '4:2:0', True)  # the pool holds at least one warm context now
    _abi.Context.__init__ = counting_init
    try:
        for _ in range(6):  # one QThread per run, as gui/worker.py does
            th = threading.Thread(target=_run, args=(img, 50, '4:2:0', True))
            th.start()
            th.join(timeout=60)
    finally:
        _abi.Context.__init__ = orig
    assert created == [], 'each run created a new context (HIP stream + scratch)'
    assert 1 <= _abi.pool_size(0) <= _abi._POOL_MAX


# The file-facing calls from two threads: what data-loader workers run.  They share the context
# pool, each context's staging buffers (grown by whichever call leased it last) and thread-local
# host tables.  Per thread and round the (H, W) of the files: growing, then shrinking.
FILE_SHAPES = [
    [[(9, 9), (17, 23)], [(65, 257), (130, 16), (40, 72), (33, 35), (31, 45)], [(3, 4)]],
    [[(31, 45), (16, 32), (33, 129)], [(200, 264), (24, 130), (64, 96), (97, 150), (17, 33), (48, 64), (24, 40)],
     [(16, 16), (37, 53)]],
]
TENSOR_SIZE = (16, 16)


def _file_jobs(t, r):
    """Thread t's round r -> [(name, call -> host result, Pillow's item 0)], in that thread's order."""
    import pjpeg_cases as pc
    from PIL import Image
    from jds import codec
    from test_jpeg_forward_cpu import image, pillow_save
    from test_jpeg_render_cpu import pillow_file, pillow_pixels
    from test_resize_cpu import pillow_draft_resize
    shapes = FILE_SHAPES[t][r]
    n = len(shapes)
    base = [pillow_file(h, w, ['4:2:0', '4:4:4', '4:2:2', 'L'][(i + t) % 4]) for i, (h, w) in enumerate(shapes)]
    prog = [pc.pillow_pair(h, w, [2, 0, 1, 'L'][(i + t) % 4], 0, 75)[1] for i, (h, w) in enumerate(shapes)]
    imgs = [image(h, w, 'noise', t) for h, w in shapes]
    modes, quals = [['4:2:0', '4:4:4', '4:2:2'][(i + t) % 3] for i in range(n)], [60 + 15 * t] * n
    plain = [pillow_save(im, m, q, False) for im, m, q in zip(imgs, modes, quals)]
    opt0 = pillow_save(imgs[0], modes[0], quals[0], True)
    dens = [[1, 2, 4, 8][i % 4] for i in range(n)]
    ops = [['none', 'rot180', 'hflip', 'vflip'][i % 4] for i in range(n)]

    def files_host(views):
        return [v.cpu().numpy().tobytes() for v in views]
    jobs = [
        ('to_rgb', lambda: codec.jpeg_batch_to_rgb(base, render='libjpeg', scale_denom=dens), pillow_pixels(base[0])),
        ('pjpeg', lambda: [v.cpu().numpy() for v in codec.pjpeg_batch_to_rgb(prog)], pc.pillow_rgb(prog[0])),
        ('transcode', lambda: files_host(codec.jpeg_batch_transcode(plain, out='device')), opt0),
        ('encode', lambda: codec.rgb_batch_to_jpeg(imgs, quals, modes, optimize=True), opt0),
        ('to_tensor', lambda: codec.jpeg_batch_to_tensor(base, TENSOR_SIZE, 'bilinear').cpu().numpy(),
         pillow_draft_resize(base[0], TENSOR_SIZE, Image.BILINEAR)),
        ('transform', lambda: codec.jpeg_batch_transform(plain, ops, trim=True), opt0),     # (item 0: 'none')
    ]
    k = (3 * t + r) % len(jobs)                              # another order in each thread and round
    return jobs[k:] + jobs[:k]


def _equal(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_two_threads_file_api_equals_single_threaded():
    from jds import _abi, build
    build.build()
    rounds = len(FILE_SHAPES[0])
    jobs = [[_file_jobs(t, r) for r in range(rounds)] for t in range(len(FILE_SHAPES))]
    refs = [[[call() for _, call, _ in rj] for rj in tj] for tj in jobs]
    for tj, tr in zip(jobs, refs):
        for rj, rr in zip(tj, tr):
            for (name, _, pil), ref in zip(rj, rr):
                assert _equal(ref[0], pil), name             # item 0 of every call is Pillow's
    results = [[None] * rounds for _ in jobs]
    errors = []
    start = threading.Barrier(len(jobs))

    def worker(t):
        try:
            start.wait()
            for r in range(rounds):
                results[t][r] = [call() for _, call, _ in jobs[t][r]]
        except Exception as e:  # surfaced in the main thread
            errors.append(e)

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(len(jobs))]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths), 'a worker thread hung'
    assert not errors, errors
    for t, tj in enumerate(jobs):
        for r, rj in enumerate(tj):
            for k, (name, _, _) in enumerate(rj):
                assert _equal(results[t][r][k], refs[t][r][k]), (t, r, name)
    assert _abi.pool_size(0) <= _abi._POOL_MAX
