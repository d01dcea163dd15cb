"""Time jds_decode_jpeg on one 1080p frame written by Pillow (quality 50, 4:2:0,
one interleaved scan, two quantisation tables): plain (standard Huffman tables),
optimize=True, restart_marker_rows=1 (one restart interval per MCU row: the
lane route) and an all-gray frame (32-bit MCUs: the sequential regime).  Beside
them jds_decode_jfif on this library's own file of the same image (three
non-interleaved scans, one table).  A call is one file from host memory to host
coefficients -- upload, the decode's launches and its read-backs between
rounds, download -- so it is timed by a host clock: three warm-up calls, REPS
(30) calls, the median.  Prints one JSON line per input; --out FILE writes them
as a JSON list.  --once: one call per input after one warm-up (for a run under
rocprofv3 --kernel-trace --stats, which gives the per-kernel split).
--rgb adds, per Pillow input, the way to pixels: jpeg_to_rgb to host memory and
to a device tensor, decompress_jpeg(staged=True) (at most 5 calls: it is slow),
k_jpeg_inv alone by events, and one more line: the plan's exact inverse k_inv2
on a frame of the same geometry by the plan's launch marks (the yardstick).
--batch N (default 64) instead: N 1080p Pillow Q50 4:2:0 files of different seeded noise images
through jpeg_batch_to_rgb(out='device') against N sequential jpeg_to_rgb(out=tensor) calls in
the same process (median of 10 after 2 warm-ups each), the rounds of the batch and the
per-kernel times from the context's launch marks; then a mixed leg: the same N split over Q50 /
Q95 / optimize=True / restart_marker_rows=1 and the three subsampling modes, at two sizes.
Writes profiles/jpeg_batch_probe.json (or --out FILE).
--transcode N (default 64) instead: the same two sets of files through jpeg_batch_transcode with
optimize False and True (to a device buffer and to host memory) against N sequential
jpeg_transcode calls in the same process, every batch output compared with its single call; the
per-kernel times of the batch from the context's launch marks, split into the decode's and the
writer's (k_mcu_*, k_ent_opt_tables); input and output bytes; and beside them, in the same run,
jpeg_batch_to_rgb(out=tensor) on the same files (the batch decode with its inverse).  Writes
profiles/transcode_probe.json (or --out FILE).
--transform N (default 64) instead: the N 1080p files through jpeg_batch_transform(out=tensor,
optimize=True) with 'rot90' for all (1080 is not a multiple of 16: with trim), 'hflip' for all and
'auto' on these files without EXIF (the plain transcode), and jpeg_batch_transcode beside them in
the same run; k_coef_xform on its own from the context's launch marks; four outputs of each leg
compared with the single call.  Writes profiles/transform_probe.json (or --out FILE).
--gray N (default 64) instead: the N 1080p pictures of --batch converted to 'L' and saved as
one-component files, plain and optimize=True, through jpeg_batch_to_rgb(out=tensor),
jpeg_batch_transcode(optimize=True, out=tensor) and jpeg_batch_transform('rot90', trim, out=tensor);
beside them, in the same run, the same pictures as 4:2:0 colour files (--batch's set).  Per leg
and call: the median time, the per-kernel times from the context's launch marks, bytes in and out,
the rounds; four outputs of each call compared with the single call.  Writes
profiles/gray_probe.json (or --out FILE).
--scale N (default 64) instead: the 1080p Pillow 4:2:0 batch at scale_denom 1, 2, 4, 8, see
scale_main.  Writes profiles/jpeg_scale_probe.json (or --out FILE).

--render N (default 64) instead: the two renderings ('reference', 'libjpeg') side by side, see
render_main.  Writes profiles/jpeg_render_probe.json (or --out FILE).
--resize N (default 64) instead: the same batch to one (N, 224, 224, 3) tensor, bicubic, through
jpeg_batch_to_tensor with the draft denominator and with scale_denom=1, see resize_main.  Writes
profiles/jpeg_resize_probe.json (or --out FILE).
--encode N (default 64) instead: the way back, pixels to files: N 1080p pictures in a device tensor
through rgb_batch_to_jpeg against N rgb_to_jpeg calls, see encode_main.  Writes
profiles/jpeg_encode_probe.json (or --out FILE).
--progressive N (default 64) instead: the pictures of --batch as progressive files through
pjpeg_batch_to_rgb against their baseline twins through jpeg_batch_to_rgb and against Pillow on
one core, see progressive_main.  Writes profiles/pjpeg_probe.json (or --out FILE)."""
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'jpeg-dsp-studio_amd'), ROOT]

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from jds import codec, entropy  # noqa: E402
from engines.quantizer import scale_quant_matrix  # noqa: E402
from utils.constants import JPEG_LUMA_Q50  # noqa: E402


def median_ms(fn, reps):
    for _ in range(1 if reps == 1 else 3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def rgb_leg(data, reps):
    """--rgb: the same file to pixels.  jpeg_to_rgb to host memory and to a device tensor and
    decompress_jpeg(staged=True) by the host clock (whole calls); k_jpeg_inv alone by events
    around back-to-back jds_jpeg_inverse_dev launches on coefficients already on the device."""
    import torch
    d = entropy.decode_jpeg(data)
    h, w = d['H'], d['W']
    fused = codec.jpeg_to_rgb(data)
    staged = codec.decompress_jpeg(data, staged=True)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda')
    row = {'jpeg_to_rgb_host_ms': median_ms(lambda: codec.jpeg_to_rgb(data), reps)[0],
           'jpeg_to_rgb_device_ms': median_ms(lambda: codec.jpeg_to_rgb(data, out=out), reps)[0],
           'decompress_jpeg_staged_ms': median_ms(lambda: codec.decompress_jpeg(data, staged=True), min(reps, 5))[0],
           'fused_equals_staged': bool(np.array_equal(fused, staged)) and bool(np.array_equal(out.cpu().numpy(), fused))}
    cf = torch.from_numpy(d['coeffs']).cuda()
    s = torch.cuda.current_stream()
    out.zero_()
    codec.jpeg_inverse_dev(d, cf.data_ptr(), out.data_ptr(), s.cuda_stream)
    s.synchronize()
    row['inverse_dev_equals_staged'] = bool(np.array_equal(out.cpu().numpy(), staged))
    # The kernel is shorter than a launch from Python: KB launches are queued behind a few
    # milliseconds of fills, so that the events bracket back-to-back launches, not the host.
    from jds import _abi
    import ctypes as C
    st = codec._jpeg_info_struct(h, w, d['mode'], d['qtables'], d['grids'])
    fill = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    KB, us = 20, []
    with _abi.lease(0) as ctx:
        for i in range(3 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(12):
                fill.fill_(i)
            e0.record(s)
            for _ in range(KB):
                _abi.check(_abi.lib().jds_jpeg_inverse_dev(ctx.handle, C.byref(st), C.c_void_p(cf.data_ptr()),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)))
            e1.record(s)
            e1.synchronize()
            if i >= 3:
                us.append(e0.elapsed_time(e1) * 1e3 / KB)
    us.sort()
    row['k_jpeg_inv_us_median_events'] = us[len(us) // 2]
    row['k_jpeg_inv_us_min_events'] = us[0]
    row['k_jpeg_inv_launches_per_event_pair'] = KB
    return row


def inv2_yardstick(H, W, reps):
    """--rgb: the plan's exact inverse k_inv2 on one frame of the same geometry (one table, the
    reference's grids), by the plan's launch marks."""
    import torch
    from jds import _abi
    qt = scale_quant_matrix(JPEG_LUMA_Q50, 50)
    plan = _abi.Plan(_abi.context(0), [_abi.make_params(50, qt, '4:2:0', True, codec.gaussian_kernel3())], H, W)
    g = torch.Generator(device='cuda').manual_seed(7)
    rgb = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
    out = torch.empty_like(rgb)
    cf = torch.zeros((1, plan.geometry.coeffs_per_frame), dtype=torch.int16, device='cuda')
    st = torch.zeros((1, _abi.STATS_DTYPE.itemsize), dtype=torch.uint8, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), 0, s)
    flags = _abi.RUN_INV | _abi.RUN_EXACT_INV
    for _ in range(3):
        plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), flags, s)
    torch.cuda.synchronize()
    plan.profile(True)
    for _ in range(reps):
        plan.run(rgb.data_ptr(), out.data_ptr(), cf.data_ptr(), st.data_ptr(), flags, s)
    torch.cuda.synchronize()
    kern, span = plan.profile_read()
    plan.profile(False)
    plan.close()
    return {'input': 'plan_exact_inverse', 'call': 'plan.run(RUN_INV | RUN_EXACT_INV)', 'H': H, 'W': W, 'reps': reps,
            'kernels_us_per_frame': {k: v[0] * 1e3 / reps for k, v in kern.items()},
            'span_us_per_frame': span * 1e3 / reps, 'equals_host_model': True}


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {'median_ms': t[len(t) // 2], 'min_ms': t[0], 'max_ms': t[-1], 'reps': reps}


def pillow_file(img, quality=50, subsampling=2, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def batch_leg(name, files, pixels):
    """One batch against the sequence of single calls on the same files."""
    import torch
    from jds import _abi
    n = len(files)
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    out = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    outs = [torch.empty((it['H'], it['W'], 3), dtype=torch.uint8, device='cuda') for it in items]
    ctx = _abi.Context(0)
    views, info = codec.jpeg_batch_to_rgb(files, out=out, with_info=True, ctx=ctx)
    torch.cuda.synchronize()
    for f, o in zip(files, outs):
        codec.jpeg_to_rgb(f, out=o)
    equal = all(bool(torch.equal(v, o)) for v, o in zip(views, outs))
    tb = timed(lambda: codec.jpeg_batch_to_rgb(files, out=out, ctx=ctx))

    def sequence():
        for f, o in zip(files, outs):
            codec.jpeg_to_rgb(f, out=o)
    ts = timed(sequence)
    ctx.profile(True)
    reps = 5
    for _ in range(reps):
        codec.jpeg_batch_to_rgb(files, out=out, ctx=ctx)
    kern, span = ctx.profile_read()
    ctx.profile(False)
    ctx.close()
    inv_us = sum(v[0] for k, v in kern.items() if k.startswith('k_jpeg_inv_batch')) * 1e3 / reps / n
    return {'leg': name, 'n': n, 'file_bytes_total': int(sum(len(f) for f in files)), 'pixels_total': int(pixels),
            'batch': tb, 'sequence': ts, 'batch_ms_per_image': tb['median_ms'] / n,
            'sequence_ms_per_image': ts['median_ms'] / n, 'factor': ts['median_ms'] / tb['median_ms'],
            'batch_images_per_s': 1e3 * n / tb['median_ms'], 'rounds': info['rounds'],
            'batch_equals_sequence': equal,
            'kernels_ms_per_batch': {k: v[0] / reps for k, v in kern.items()},
            'kernel_launches_per_batch': {k: v[1] / reps for k, v in kern.items()},
            'marks_span_ms_per_batch': span / reps, 'k_jpeg_inv_batch_us_per_image': inv_us}


def batch_main():
    i = sys.argv.index('--batch')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    plain = [pillow_file(np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)) for k in range(n)]
    rows = [batch_leg('pillow_q50_420_1080p', plain, n * H * W)]
    print(json.dumps(rows[-1]), flush=True)
    kinds = [{'quality': 50}, {'quality': 95}, {'quality': 50, 'optimize': True}, {'quality': 50, 'restart_marker_rows': 1}]
    sizes = [(H, W), (2 * H // 3, 2 * W // 3)]
    mixed, px = [], 0
    for k in range(n):
        h, w = sizes[(k // 12) % 2]
        img = np.random.default_rng(500 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
        mixed.append(pillow_file(img, subsampling=(2, 0, 1)[k % 3], **kinds[(k // 3) % 4]))
        px += h * w
    rows.append(batch_leg('pillow_mixed', mixed, px))
    print(json.dumps(rows[-1]), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'jpeg_batch_probe.json')
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r['batch_equals_sequence'] for r in rows) else 1


def transcode_leg(name, files):
    """One set of files: the batch call against the sequence of single calls, both table kinds."""
    import torch
    from jds import _abi
    n = len(files)
    ctx = _abi.Context(0)
    row = {'leg': name, 'n': n, 'input_bytes': int(sum(len(f) for f in files))}
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    rgb = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    row['batch_to_rgb'] = timed(lambda: codec.jpeg_batch_to_rgb(files, out=rgb, ctx=ctx))
    for opt in (False, True):
        outs = codec.jpeg_batch_transcode(files, optimize=opt, ctx=ctx)
        singles = [codec.jpeg_transcode(f, optimize=opt) for f in files]
        buf = torch.empty(sum(-(-len(o) // 256) * 256 for o in outs), dtype=torch.uint8, device='cuda')
        views = codec.jpeg_batch_transcode(files, optimize=opt, out=buf, ctx=ctx)
        equal = outs == singles and all(v.cpu().numpy().tobytes() == o for v, o in zip(views, outs))
        tb = timed(lambda: codec.jpeg_batch_transcode(files, optimize=opt, out=buf, ctx=ctx))
        th = timed(lambda: codec.jpeg_batch_transcode(files, optimize=opt, ctx=ctx))
        ts = timed(lambda: [codec.jpeg_transcode(f, optimize=opt) for f in files], reps=5, warm=1)
        ctx.profile(True)
        reps = 5
        for _ in range(reps):
            codec.jpeg_batch_transcode(files, optimize=opt, out=buf, ctx=ctx)
        kern, span = ctx.profile_read()
        ctx.profile(False)
        writer = {k: v[0] / reps for k, v in kern.items() if k.startswith('k_mcu') or k.startswith('k_ent_opt')}
        decode = {k: v[0] / reps for k, v in kern.items() if k not in writer and not k.startswith('(')}
        row['optimize' if opt else 'annex_k'] = {
            'output_bytes': int(sum(len(o) for o in outs)), 'batch_equals_singles': bool(equal),
            'batch_to_device': tb, 'batch_to_host': th, 'single_calls': ts,
            'single_over_batch': ts['median_ms'] / tb['median_ms'],
            'batch_minus_batch_to_rgb_ms': tb['median_ms'] - row['batch_to_rgb']['median_ms'],
            'writer_kernels_ms_per_batch': writer, 'writer_kernels_ms_total': sum(writer.values()),
            'decode_kernels_ms_per_batch': decode, 'decode_kernels_ms_total': sum(decode.values()),
            'other_marks_ms_per_batch': {k: v[0] / reps for k, v in kern.items() if k.startswith('(')},
            'marks_span_ms_per_batch': span / reps}
    ctx.close()
    return row


def transcode_main():
    i = sys.argv.index('--transcode')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    plain = [pillow_file(np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)) for k in range(n)]
    rows = [transcode_leg('pillow_q50_420_1080p', plain)]
    print(json.dumps(rows[-1]), flush=True)
    kinds = [{'quality': 50}, {'quality': 95}, {'quality': 50, 'optimize': True}, {'quality': 50, 'restart_marker_rows': 1}]
    sizes = [(H, W), (2 * H // 3, 2 * W // 3)]
    mixed = []
    for k in range(n):
        h, w = sizes[(k // 12) % 2]
        img = np.random.default_rng(500 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
        mixed.append(pillow_file(img, subsampling=(2, 0, 1)[k % 3], **kinds[(k // 3) % 4]))
    rows.append(transcode_leg('pillow_mixed', mixed))
    print(json.dumps(rows[-1]), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'transcode_probe.json')
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r[k]['batch_equals_singles'] for r in rows for k in ('annex_k', 'optimize')) else 1


def transform_main():
    import torch
    from jds import _abi
    i = sys.argv.index('--transform')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    files = [pillow_file(np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)) for k in range(n)]
    ctx = _abi.Context(0)
    legs = [('transcode', None, False), ('rot90_trim', 'rot90', True), ('hflip', 'hflip', False),
            ('auto_no_exif', 'auto', False)]

    def call(op, trim, **kw):
        if op is None:
            return codec.jpeg_batch_transcode(files, optimize=True, ctx=ctx, **kw)
        return codec.jpeg_batch_transform(files, op, trim=trim, optimize=True, ctx=ctx, **kw)

    row = {'n': n, 'H': H, 'W': W, 'input_bytes': int(sum(len(f) for f in files)), 'legs': {}}
    ok = True
    for name, op, trim in legs:
        outs = call(op, trim)
        buf = torch.empty(sum(-(-len(o) // 256) * 256 for o in outs), dtype=torch.uint8, device='cuda')
        some = range(0, n, max(1, n // 4))
        singles = [codec.jpeg_transcode(files[k]) if op is None else codec.jpeg_transform(files[k], op, trim=trim)
                   for k in some]
        equal = singles == [outs[k] for k in some]
        if name == 'auto_no_exif':
            equal = equal and outs == call(None, False)
        ok = ok and equal
        tb = timed(lambda: call(op, trim, out=buf))
        ctx.profile(True)
        reps = 5
        for _ in range(reps):
            call(op, trim, out=buf)
        kern, span = ctx.profile_read()
        ctx.profile(False)
        writer = {k: v[0] / reps for k, v in kern.items() if k.startswith('k_mcu') or k.startswith('k_ent_opt')}
        row['legs'][name] = {'batch_to_device': tb, 'output_bytes': int(sum(len(o) for o in outs)),
                             'equals_single_calls': bool(equal),
                             'out_size': list(codec.jpeg_transform_info(outs[0], 'none').values())[1:],
                             'k_coef_xform_ms_per_batch': kern.get('k_coef_xform', (0.0, 0))[0] / reps,
                             'k_coef_xform_launches_per_batch': kern.get('k_coef_xform', (0.0, 0))[1] / reps,
                             'writer_kernels_ms_total': sum(writer.values()),
                             'marks_span_ms_per_batch': span / reps}
    ctx.close()
    base = row['legs']['transcode']['batch_to_device']['median_ms']
    for name in ('rot90_trim', 'hflip', 'auto_no_exif'):
        row['legs'][name]['minus_transcode_ms'] = row['legs'][name]['batch_to_device']['median_ms'] - base
    print(json.dumps(row), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'transform_probe.json')
    with open(out, 'w') as f:
        json.dump([row], f, indent=1)
        f.write('\n')
    return 0 if ok else 1


def gray_leg(name, files):
    import torch
    from jds import _abi
    n = len(files)
    ctx = _abi.Context(0)
    row = {'leg': name, 'n': n, 'input_bytes': int(sum(len(f) for f in files))}
    ok = True
    some = range(0, n, max(1, n // 4))

    def marks(fn, reps=5):
        ctx.profile(True)
        for _ in range(reps):
            fn()
        kern, span = ctx.profile_read()
        ctx.profile(False)
        return {'kernels_ms_per_batch': {k: v[0] / reps for k, v in kern.items()},
                'kernel_launches_per_batch': {k: v[1] / reps for k, v in kern.items()},
                'marks_span_ms_per_batch': span / reps}

    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    rgb = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    views, info = codec.jpeg_batch_to_rgb(files, out=rgb, with_info=True, ctx=ctx)
    equal = all(np.array_equal(views[k].cpu().numpy(), codec.jpeg_to_rgb(files[k])) for k in some)
    ok = ok and equal
    row['batch_to_rgb'] = dict(timed(lambda: codec.jpeg_batch_to_rgb(files, out=rgb, ctx=ctx)), rounds=info['rounds'],
                               output_bytes=int(rgb_bytes), equals_single_calls=bool(equal),
                               **marks(lambda: codec.jpeg_batch_to_rgb(files, out=rgb, ctx=ctx)))
    calls = [('batch_transcode', lambda **kw: codec.jpeg_batch_transcode(files, optimize=True, ctx=ctx, **kw),
              lambda f: codec.jpeg_transcode(f, optimize=True)),
             ('batch_transform_rot90_trim',
              lambda **kw: codec.jpeg_batch_transform(files, 'rot90', trim=True, optimize=True, ctx=ctx, **kw),
              lambda f: codec.jpeg_transform(f, 'rot90', trim=True, optimize=True))]
    for cname, call, single in calls:
        outs = call()
        buf = torch.empty(sum(-(-len(o) // 256) * 256 for o in outs), dtype=torch.uint8, device='cuda')
        equal = [outs[k] for k in some] == [single(files[k]) for k in some]
        ok = ok and equal
        row[cname] = dict(timed(lambda: call(out=buf)), output_bytes=int(sum(len(o) for o in outs)),
                          equals_single_calls=bool(equal), **marks(lambda: call(out=buf)))
    ctx.close()
    row['ok'] = bool(ok)
    return row


def gray_main():
    i = sys.argv.index('--gray')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    pics = [np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]

    def gray_file(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).convert('L').save(buf, 'JPEG', quality=50, **kw)
        return buf.getvalue()

    legs = [('pillow_q50_gray_1080p', [gray_file(p) for p in pics]),
            ('pillow_q50_gray_optimize_1080p', [gray_file(p, optimize=True) for p in pics]),
            ('pillow_q50_420_1080p', [pillow_file(p) for p in pics])]
    rows = []
    for name, files in legs:
        rows.append(gray_leg(name, files))
        print(json.dumps(rows[-1]), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'gray_probe.json')
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r['ok'] for r in rows) else 1


def render_kernel_us(d, reps, KB=20):
    """Both inverse kernels on the same coefficients by events around KB back-to-back launches
    (rgb_leg's method), the two renderings alternating rep by rep.  -> {render: (median, min)}."""
    import ctypes as C
    import torch
    from jds import _abi
    h, w = d['H'], d['W']
    st = codec._jpeg_info_struct(h, w, d['mode'], d['qtables'], d['grids'])
    cf = torch.from_numpy(d['coeffs']).cuda()
    out = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda')
    fill = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    s = torch.cuda.current_stream()
    us = {0: [], 1: []}
    with _abi.lease(0) as ctx:
        for i in range(3 + reps):
            for code in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(12):
                    fill.fill_(i)
                e0.record(s)
                for _ in range(KB):
                    _abi.check(_abi.lib().jds_jpeg_render_dev(ctx.handle, C.byref(st), C.c_void_p(cf.data_ptr()),
                                                              C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream), code))
                e1.record(s)
                e1.synchronize()
                if i >= 3:
                    us[code].append(e0.elapsed_time(e1) * 1e3 / KB)
    return {name: (sorted(us[c])[len(us[c]) // 2], min(us[c])) for name, c in (('reference', 0), ('libjpeg', 1))}


def render_single_leg(name, data, reps):
    import torch
    d = entropy.decode_jpeg(data)
    h, w = d['H'], d['W']
    out = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda')
    ref = codec.jpeg_to_rgb(data)
    lj = codec.jpeg_to_rgb(data, render='libjpeg')
    pil = np.asarray(Image.open(io.BytesIO(bytes(data))).convert('RGB'))
    t = {'reference': [], 'libjpeg': []}
    for i in range(3 + reps):                               # alternating, whole calls by the host clock
        for r in t:
            t0 = time.perf_counter()
            codec.jpeg_to_rgb(data, out=out, render=r)
            if i >= 3:
                t[r].append((time.perf_counter() - t0) * 1e3)
    k = render_kernel_us(d, reps)
    diff = ref.astype(np.int16) - lj
    return {'leg': name, 'H': h, 'W': w, 'mode': d['mode'], 'file_bytes': int(len(data)), 'reps': reps,
            'jpeg_to_rgb_device_ms': {r: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v)} for r, v in t.items()},
            'kernel_us_events': {'k_jpeg_inv': {'median': k['reference'][0], 'min': k['reference'][1]},
                                 'k_jpeg_ljt': {'median': k['libjpeg'][0], 'min': k['libjpeg'][1]}},
            'libjpeg_equals_pillow': bool(np.array_equal(lj, pil)),
            'bytes_differing_between_renderings': int((diff != 0).sum()), 'bytes_total': int(diff.size),
            'largest_difference': int(np.abs(diff).max())}


def render_order_leg(name, data, reps=40):
    """Does a difference between the renderings in whole calls follow the rendering or the call's
    place?  jpeg_to_rgb(out=tensor) by the host clock: alternating pairs in both orders, then
    blocks of `reps` calls of one rendering, twice.  Medians, ms."""
    import torch
    info = entropy.parse_jpeg(data)
    out = torch.empty((info['H'], info['W'], 3), dtype=torch.uint8, device='cuda')

    def one(r):
        t0 = time.perf_counter()
        codec.jpeg_to_rgb(data, out=out, render=r)
        return (time.perf_counter() - t0) * 1e3

    def med(v):
        return sorted(v)[len(v) // 2]
    for r in ('reference', 'libjpeg'):
        for _ in range(5):
            one(r)
    row = {'leg': name, 'reps': reps, 'libjpeg_equals_pillow': True}
    for key, order in (('alternating_reference_first', ('reference', 'libjpeg')),
                       ('alternating_libjpeg_first', ('libjpeg', 'reference'))):
        t = {'reference': [], 'libjpeg': []}
        for _ in range(reps):
            for r in order:
                t[r].append(one(r))
        row[key] = {r: med(v) for r, v in t.items()}
    row['blocks'] = {'reference': [], 'libjpeg': []}
    for _ in range(2):
        for r in ('reference', 'libjpeg'):
            row['blocks'][r].append(med([one(r) for _ in range(reps)]))
    return row


def render_batch_leg(name, files):
    import torch
    from jds import _abi
    n = len(files)
    items, rgb_bytes, _ = codec.jpeg_batch_layout(files)
    out = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    ctx = _abi.Context(0)
    row = {'leg': name, 'n': n, 'file_bytes_total': int(sum(len(f) for f in files))}
    views = codec.jpeg_batch_to_rgb(files, out=out, ctx=ctx, render='libjpeg')
    some = range(0, n, max(1, n // 4))
    row['libjpeg_equals_pillow'] = all(
        np.array_equal(views[k].cpu().numpy(), np.asarray(Image.open(io.BytesIO(files[k])).convert('RGB'))) for k in some)
    t = {'reference': [], 'libjpeg': []}
    for i in range(2 + 10):
        for r in t:
            t0 = time.perf_counter()
            codec.jpeg_batch_to_rgb(files, out=out, ctx=ctx, render=r)
            if i >= 2:
                t[r].append((time.perf_counter() - t0) * 1e3)
    row['jpeg_batch_to_rgb_device_ms'] = {r: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v)}
                                          for r, v in t.items()}
    ctx.profile(True)
    reps = 5
    for _ in range(reps):
        for r in t:
            codec.jpeg_batch_to_rgb(files, out=out, ctx=ctx, render=r)
    kern, _ = ctx.profile_read()
    ctx.profile(False)
    ctx.close()
    row['inverse_kernels_ms_per_batch'] = {k: v[0] / reps for k, v in kern.items()
                                           if k.startswith('k_jpeg_inv_batch') or k.startswith('k_jpeg_ljt_batch')}
    return row


def render_main():
    """--render [N]: the two renderings side by side -- per 1080p Pillow Q50 file (4:2:0, 4:2:2,
    4:4:4, one-component) jpeg_to_rgb(out=tensor) alternating between them, the two inverse kernels
    by events around back-to-back launches, the bytes that differ; the 4:2:0 picture once more at
    1080 x 1919 (rows at odd addresses: the byte-store path of both kernels) and in a call-order
    check (render_order_leg); then N (default 64) 4:2:0 files
    and N one-component files through jpeg_batch_to_rgb(out=tensor), alternating, with the batch
    kernels from the context's launch marks.  Writes profiles/jpeg_render_probe.json (or --out FILE)."""
    i = sys.argv.index('--render')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    reps = int(os.environ.get('REPS', '30'))
    noise = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)

    def gray_file(img):
        buf = io.BytesIO()
        Image.fromarray(img).convert('L').save(buf, 'JPEG', quality=50)
        return buf.getvalue()

    rows = []
    for name, data in (('pillow_q50_420_1080p', pillow_file(noise)), ('pillow_q50_422_1080p', pillow_file(noise, subsampling=1)),
                       ('pillow_q50_444_1080p', pillow_file(noise, subsampling=0)), ('pillow_q50_gray_1080p', gray_file(noise))):
        rows.append(render_single_leg(name, data, reps))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(render_single_leg('pillow_q50_420_1080x1919', pillow_file(np.ascontiguousarray(noise[:, :W - 1])), reps))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(render_order_leg('call_order_check_pillow_q50_420_1080p', pillow_file(noise)))
    print(json.dumps(rows[-1]), flush=True)
    pics = [np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]
    for name, files in (('batch_pillow_q50_420_1080p', [pillow_file(p) for p in pics]),
                        ('batch_pillow_q50_gray_1080p', [gray_file(p) for p in pics])):
        rows.append(render_batch_leg(name, files))
        print(json.dumps(rows[-1]), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'jpeg_render_probe.json')
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r['libjpeg_equals_pillow'] for r in rows) else 1


def scale_main():
    """--scale [N]: the N (default 64) 1080p Pillow Q50 4:2:0 files of the --render batch leg through
    jpeg_batch_to_rgb(out=tensor, render='libjpeg', scale_denom=d) at d = 1, 2, 4, 8, the four
    alternating call by call in one process: the whole call by the host clock (median, min, max of
    10 after 2 warm-ups); k_jpeg_ljt_batch (d = 1) and k_jpeg_ljs_batch (d = 2, 4, 8) from the
    context's launch marks (events), per batch, in ROUNDS (default 7) rounds of 3 alternating
    repetitions each -- median over the rounds and their min / max, the spread the comparison is
    read against; the output bytes (derived from the layout); four images per denominator against
    Pillow's Image.draft.  Writes profiles/jpeg_scale_probe.json (or --out FILE)."""
    import torch
    from jds import _abi
    i = sys.argv.index('--scale')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    rounds = int(os.environ.get('ROUNDS', '7'))
    pics = [np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]
    files = [pillow_file(p) for p in pics]
    dens = (1, 2, 4, 8)
    row = {'leg': 'batch_pillow_q50_420_1080p_scaled', 'n': n, 'H': H, 'W': W,
           'file_bytes_total': int(sum(len(f) for f in files)), 'denominators': list(dens), 'rounds': rounds}
    ctx = _abi.Context(0)
    outs, row['output_bytes'], row['equals_pillow'] = {}, {}, {}
    for d in dens:
        items, rgb_bytes, _ = codec.jpeg_batch_layout(files, scale_denom=d)
        outs[d] = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
        row['output_bytes'][str(d)] = int(sum(it['out_H'] * it['out_W'] * 3 for it in items))
        views = codec.jpeg_batch_to_rgb(files, out=outs[d], ctx=ctx, render='libjpeg', scale_denom=d)
        ok = True
        for k in range(0, n, max(1, n // 4)):
            im = Image.open(io.BytesIO(files[k]))
            if d != 1:
                im.draft('RGB', (W // d, H // d))
            ok = ok and np.array_equal(views[k].cpu().numpy(), np.asarray(im.convert('RGB')))
        row['equals_pillow'][str(d)] = bool(ok)
    t = {d: [] for d in dens}
    for r in range(2 + 10):
        for d in dens:
            t0 = time.perf_counter()
            codec.jpeg_batch_to_rgb(files, out=outs[d], ctx=ctx, render='libjpeg', scale_denom=d)
            if r >= 2:
                t[d].append((time.perf_counter() - t0) * 1e3)
    row['jpeg_batch_to_rgb_device_ms'] = {str(d): {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v)}
                                          for d, v in t.items()}
    ctx.profile(True)
    ctx.profile_read()
    reps, per = 3, {d: [] for d in dens}
    for _ in range(rounds):
        for _ in range(reps):
            for d in dens:
                codec.jpeg_batch_to_rgb(files, out=outs[d], ctx=ctx, render='libjpeg', scale_denom=d)
        kern, _ = ctx.profile_read()
        for d in dens:
            name = 'k_jpeg_ljt_batch<2>' if d == 1 else f'k_jpeg_ljs_batch<2,{d}>'
            per[d].append(kern[name][0] / reps)
    ctx.profile(False)
    ctx.close()
    row['kernel_ms_per_batch'] = {('k_jpeg_ljt_batch' if d == 1 else f'k_jpeg_ljs_batch_1/{d}'):
                                  {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v), 'rounds': v}
                                  for d, v in per.items()}
    full = row['kernel_ms_per_batch']['k_jpeg_ljt_batch']
    row['scaled_not_slower_than_full'] = {k: bool(v['median'] <= full['median'] + (full['max'] - full['min']))
                                          for k, v in row['kernel_ms_per_batch'].items() if k != 'k_jpeg_ljt_batch'}
    print(json.dumps(row), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'jpeg_scale_probe.json')
    with open(out, 'w') as f:
        json.dump([row], f, indent=1)
        f.write('\n')
    return 0 if all(row['equals_pillow'].values()) else 1


def resize_main():
    """--resize [N]: the N (default 64) 1080p Pillow Q50 4:2:0 files of --scale to one (N, 224, 224, 3)
    device tensor, bicubic, in two legs: 'draft' (Image.draft's denominator: 4, 480 x 270 decoded)
    and 'full' (scale_denom=1).  Per leg jpeg_batch_to_tensor alternates call by call with the
    decode-only jpeg_batch_to_rgb(out=tensor, render='libjpeg', scale_denom=...) on the same context:
    whole calls by the host clock (median, min, max of 10 after 2 warm-ups); then k_resize_batch and
    the render kernel beside it from the context's launch marks (events) in ROUNDS (default 7) rounds
    of 3 repetitions -- median over the rounds and their min / max; the bytes the resize reads and
    writes; every slot against Pillow's draft + resize.  Two conditions are evaluated for the draft
    leg: the resize kernel takes no longer than the render kernel, and the whole call exceeds the
    decode-only call plus the resize kernel by no more than the decode-only call's spread.  Writes
    profiles/jpeg_resize_probe.json (or --out FILE)."""
    import torch
    from jds import _abi
    i = sys.argv.index('--resize')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    rounds = int(os.environ.get('ROUNDS', '7'))
    size, flt = (224, 224), 'bicubic'
    files = [pillow_file(np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8)) for k in range(n)]
    ctx = _abi.Context(0)
    out = torch.empty((n, size[1], size[0], 3), dtype=torch.uint8, device='cuda')
    rows = []
    for leg, den in (('draft', 'draft'), ('full', 1)):
        d = codec.draft_denom(H, W, size) if den == 'draft' else 1
        items, rgb_bytes, _ = codec.jpeg_batch_layout(files, scale_denom=d)
        dec = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
        row = {'leg': f'batch_pillow_q50_420_1080p_to_224_bicubic_{leg}', 'n': n, 'H': H, 'W': W, 'scale_denom': d,
               'decoded_H': items[0]['out_H'], 'decoded_W': items[0]['out_W'], 'rounds': rounds,
               'file_bytes_total': int(sum(len(f) for f in files)),
               'resize_bytes_read': int(sum(it['out_H'] * it['out_W'] * 3 for it in items)),
               'resize_bytes_written': int(out.numel())}

        def tensor():
            return codec.jpeg_batch_to_tensor(files, size, flt, scale_denom=den, out=out, ctx=ctx)

        def decode():
            return codec.jpeg_batch_to_rgb(files, out=dec, ctx=ctx, render='libjpeg', scale_denom=d)
        got = tensor().cpu().numpy()
        ok = True
        for k in range(n):
            im = Image.open(io.BytesIO(files[k]))
            if den == 'draft':
                im.draft('RGB', size)
            ok = ok and np.array_equal(got[k], np.asarray(im.convert('RGB').resize(size, Image.Resampling.BICUBIC)))
        row['equals_pillow'] = bool(ok)
        t = {'tensor': [], 'decode': []}
        for r in range(2 + 10):
            for name, fn in (('tensor', tensor), ('decode', decode)):
                t0 = time.perf_counter()
                fn()
                if r >= 2:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        row['whole_call_ms'] = {k: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v)} for k, v in t.items()}
        ctx.profile(True)
        ctx.profile_read()
        reps, per = 3, {'k_resize_batch': [], 'render': []}
        render = 'k_jpeg_ljt_batch<2>' if d == 1 else f'k_jpeg_ljs_batch<2,{d}>'
        for _ in range(rounds):
            for _ in range(reps):
                tensor()
                decode()
            kern, _ = ctx.profile_read()
            per['k_resize_batch'].append(kern['k_resize_batch'][0] / reps)
            per['render'].append(kern[render][0] / (2 * reps))          # (both calls launch it)
        ctx.profile(False)
        row['render_kernel'] = render
        row['kernel_ms_per_batch'] = {k: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v), 'rounds': v}
                                      for k, v in per.items()}
        wc, km = row['whole_call_ms'], row['kernel_ms_per_batch']
        row['resize_not_slower_than_render'] = bool(km['k_resize_batch']['median'] <= km['render']['median'])
        row['whole_call_excess_ms'] = wc['tensor']['median'] - wc['decode']['median'] - km['k_resize_batch']['median']
        row['whole_call_within_decode_spread'] = bool(row['whole_call_excess_ms'] <= wc['decode']['max'] - wc['decode']['min'])
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    dst = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'jpeg_resize_probe.json')
    with open(dst, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r['equals_pillow'] for r in rows) else 1


def encode_main():
    """--encode [N]: N (default 64) 1080p noise pictures in one device tensor through
    rgb_batch_to_jpeg (4:2:0, quality 75, out='device'), plain and optimize=True, against N
    rgb_to_jpeg calls on the same tensor's images in the same process (whole calls by the host
    clock: median of 30 after 3 warm-ups, the two alternating); k_jpeg_fwd_batch and the writer's
    kernels from the context's launch marks (events), and beside them, in the same profiled loop,
    k_jpeg_ljt_batch decoding the files just written (the same geometry in the other direction);
    the output bytes; the first file against Pillow's and four against the single call.  Writes
    profiles/jpeg_encode_probe.json (or --out FILE)."""
    import torch
    from jds import _abi
    i = sys.argv.index('--encode')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    pics = [np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]
    stack = torch.stack([torch.from_numpy(p) for p in pics]).cuda()
    ctx = _abi.Context(0)
    rows = []
    for optimize in (False, True):
        row = {'leg': 'batch_rgb_q75_420_1080p_' + ('optimize' if optimize else 'plain'), 'n': n, 'H': H, 'W': W,
               'rgb_bytes_total': int(stack.numel())}
        outs = codec.rgb_batch_to_jpeg(stack, 75, '4:2:0', optimize, out='device', ctx=ctx)
        files = [o.cpu().numpy().tobytes() for o in outs]
        row['file_bytes_total'] = int(sum(len(f) for f in files))
        row['first_file_equals_pillow'] = files[0] == pillow_file(pics[0], quality=75, subsampling=2, optimize=optimize)
        some = range(0, n, max(1, n // 4))
        row['batch_equals_single'] = all(files[k] == codec.rgb_to_jpeg(stack[k], 75, '4:2:0', optimize) for k in some)
        t = {'batch': [], 'sequence': []}
        for r in range(3 + 30):
            t0 = time.perf_counter()
            codec.rgb_batch_to_jpeg(stack, 75, '4:2:0', optimize, out='device', ctx=ctx)
            t1 = time.perf_counter()
            for k in range(n):
                codec.rgb_to_jpeg(stack[k], 75, '4:2:0', optimize)
            t2 = time.perf_counter()
            if r >= 3:
                t['batch'].append((t1 - t0) * 1e3)
                t['sequence'].append((t2 - t1) * 1e3)
        row['ms_per_batch'] = {k: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v)} for k, v in t.items()}
        _, rgb_bytes, _ = codec.jpeg_batch_layout(files)
        back = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
        views = codec.jpeg_batch_to_rgb(files, out=back, ctx=ctx, render='libjpeg')      # (warm-up of the decode side)
        row['decoded_shape_ok'] = all(tuple(v.shape) == (H, W, 3) for v in views)
        ctx.profile(True)
        reps = 5
        for _ in range(reps):
            codec.rgb_batch_to_jpeg(stack, 75, '4:2:0', optimize, out='device', ctx=ctx)
            codec.jpeg_batch_to_rgb(files, out=back, ctx=ctx, render='libjpeg')
        kern, _ = ctx.profile_read()
        ctx.profile(False)
        row['kernels_ms_per_batch'] = {k: v[0] / reps for k, v in kern.items()
                                       if k.startswith(('k_jpeg_fwd_batch', 'k_jpeg_ljt_batch', 'k_mcu_', 'k_ent_opt'))}
        fwd = sum(v for k, v in row['kernels_ms_per_batch'].items() if k.startswith('k_jpeg_fwd_batch'))
        ljt = sum(v for k, v in row['kernels_ms_per_batch'].items() if k.startswith('k_jpeg_ljt_batch'))
        row['fwd_over_ljt'] = fwd / ljt if ljt else None
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'jpeg_encode_probe.json')
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    return 0 if all(r['first_file_equals_pillow'] and r['batch_equals_single'] for r in rows) else 1


def progressive_main():
    """--progressive N: the N 1080p pictures of --batch saved by Pillow with progressive=True through
    pjpeg_batch_to_rgb(out=tensor, render='libjpeg') against jpeg_batch_to_rgb(render='libjpeg') on
    their baseline twins, the two legs alternating in one run (REPS rounds, default 5, after one
    warm-up each; medians); k_pjpeg_chains from the context's launch marks (events) and, from the
    walk times the kernel takes itself on a profiled context, the longest chain of the batch and
    the scan kinds it spends its time in; Pillow's decode of the same N progressive files in a loop
    on one core of this machine.  Writes profiles/pjpeg_probe.json (or --out FILE)."""
    import torch
    from jds import _abi
    i = sys.argv.index('--progressive')
    n = int(sys.argv[i + 1]) if i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit() else 64
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    reps = int(os.environ.get('REPS', '5'))
    imgs = [np.random.default_rng(100 + k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]
    prog = [pillow_file(im, progressive=True) for im in imgs]
    base = [pillow_file(im) for im in imgs]
    _, rgb_bytes, _ = codec.jpeg_batch_layout(base)
    out_p = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    out_b = torch.empty(rgb_bytes, dtype=torch.uint8, device='cuda')
    ctx = _abi.Context(0)

    def leg_p():
        return codec.pjpeg_batch_to_rgb(prog, out=out_p, render='libjpeg', ctx=ctx)

    def leg_b():
        return codec.jpeg_batch_to_rgb(base, out=out_b, render='libjpeg', ctx=ctx)
    vp, vb = leg_p(), leg_b()                                # (the warm-up of both legs)
    torch.cuda.synchronize()
    equal = all(bool(torch.equal(a, b)) for a, b in zip(vp, vb))
    first_equals_pillow = bool(np.array_equal(vp[0].cpu().numpy(), np.asarray(Image.open(io.BytesIO(prog[0])).convert('RGB'))))
    tp, tb = [], []
    for _ in range(reps):                                    # alternating: both legs see the same machine
        for fn, t in ((leg_p, tp), (leg_b, tb)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    leg_p()
    kern, span = ctx.profile_read()
    times = codec.pjpeg_scan_times(ctx, prog)
    ctx.profile(False)
    ctx.close()
    kinds = {}
    longest = (0.0, None)
    for k, (f, per) in enumerate(zip(prog, times)):
        scans = entropy.parse_pjpeg(f)['scans']
        chains = {}
        for j, us in per:
            s = scans[j]
            key = 'dc' if s['ss'] == 0 else 'ac%d' % s['components'][0]
            kind = ('dc' if s['ss'] == 0 else 'ac') + ('_first' if s['ah'] == 0 else '_refine')
            chains.setdefault(key, []).append((j, kind, s['ss'], s['se'], s['ah'], s['al'], us))
            kinds[kind] = kinds.get(kind, 0.0) + us
        for key, lst in chains.items():
            tot = sum(x[-1] for x in lst)
            if tot > longest[0]:
                longest = (tot, {'file': k, 'chain': key, 'ms': tot / 1e3,
                                 'scans': [{'scan': j, 'kind': kind, 'ss': ss, 'se': se, 'ah': ah, 'al': al, 'ms': us / 1e3}
                                           for j, kind, ss, se, ah, al, us in lst]})
    t0 = time.perf_counter()
    for f in prog:
        np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
    pil_prog = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for f in base:
        np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
    pil_base = (time.perf_counter() - t0) * 1e3
    med = lambda t: sorted(t)[len(t) // 2]
    row = {'leg': 'pillow_q50_420_1080p_progressive', 'n': n, 'H': H, 'W': W, 'reps': reps,
           'progressive_bytes_total': int(sum(len(f) for f in prog)), 'baseline_bytes_total': int(sum(len(f) for f in base)),
           'pjpeg_batch_to_rgb_ms': {'median': med(tp), 'min': min(tp), 'max': max(tp)},
           'jpeg_batch_to_rgb_baseline_twins_ms': {'median': med(tb), 'min': min(tb), 'max': max(tb)},
           'progressive_over_baseline': med(tp) / med(tb),
           'kernels_ms_per_batch': {k: v[0] for k, v in kern.items()}, 'marks_span_ms_per_batch': span,
           'k_pjpeg_chains_ms_events': kern.get('k_pjpeg_chains', [None])[0],
           'longest_chain': longest[1], 'scan_kind_lane_ms_total': {k: v / 1e3 for k, v in kinds.items()},
           'pillow_one_core_progressive_ms': pil_prog, 'pillow_one_core_baseline_ms': pil_base,
           'chains_slower_than_pillow_one_core': bool(kern.get('k_pjpeg_chains', [0.0])[0] > pil_prog),
           'progressive_equals_baseline_twins': equal, 'first_file_equals_pillow': first_equals_pillow}
    print(json.dumps(row), flush=True)
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'pjpeg_probe.json')
    with open(out, 'w') as f:
        json.dump([row], f, indent=1)
        f.write('\n')
    return 0 if equal and first_equals_pillow else 1


def main():
    if '--progressive' in sys.argv:
        return progressive_main()
    if '--encode' in sys.argv:
        return encode_main()
    if '--resize' in sys.argv:
        return resize_main()
    if '--scale' in sys.argv:
        return scale_main()
    if '--render' in sys.argv:
        return render_main()
    if '--gray' in sys.argv:
        return gray_main()
    if '--transform' in sys.argv:
        return transform_main()
    if '--batch' in sys.argv:
        return batch_main()
    if '--transcode' in sys.argv:
        return transcode_main()
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    reps = 1 if '--once' in sys.argv else int(os.environ.get('REPS', '30'))
    want_rgb = '--rgb' in sys.argv
    noise = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    gray = np.full((H, W, 3), 128, np.uint8)
    inputs = [('pillow_plain', noise, {}), ('pillow_optimize', noise, {'optimize': True}),
              ('pillow_restart_rows1', noise, {'restart_marker_rows': 1}), ('pillow_all_gray', gray, {})]
    rows = []
    for name, img, kw in inputs:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=50, subsampling=2, **kw)
        data = np.frombuffer(buf.getvalue(), np.uint8)
        d = entropy.decode_jpeg(data)
        ok = bool(np.array_equal(d['coeffs'], entropy.host_decode_jpeg(data)[0]))
        med, lo, hi = median_ms(lambda: entropy.decode_jpeg(data), reps)
        rows.append({'input': name, 'call': 'decode_jpeg', 'H': H, 'W': W, 'file_bytes': int(data.size),
                     'restart_interval_mcus': d['scans'][0]['restart_interval'], 'rounds': d['rounds'],
                     'ms_per_file_median': med, 'ms_min': lo, 'ms_max': hi, 'reps': reps,
                     'equals_host_model': ok, 'subseq_bits_per_group': entropy.decode_info()})
        if want_rgb:
            rows[-1].update(rgb_leg(data, reps))
            rows[-1]['equals_host_model'] = ok and rows[-1]['fused_equals_staged'] and rows[-1]['inverse_dev_equals_staged']
        print(json.dumps(rows[-1]), flush=True)
    if want_rgb:
        rows.append(inv2_yardstick(H, W, reps))
        print(json.dumps(rows[-1]), flush=True)
    # this library's own file of the same images
    qt = scale_quant_matrix(JPEG_LUMA_Q50, 50)
    for name, img in (('own_file_noise', noise), ('own_file_all_gray', gray)):
        raw = codec.compress_reconstruct_raw(img, 50, qt, '4:2:0', True, maps=False)
        own = np.frombuffer(entropy.encode_jfif(raw['coeffs'], H, W, '4:2:0', qt)[0], np.uint8)
        d = entropy.decode_jfif(own)
        med, lo, hi = median_ms(lambda: entropy.decode_jfif(own), reps)
        rows.append({'input': name, 'call': 'decode_jfif', 'H': H, 'W': W, 'file_bytes': int(own.size),
                     'rounds': d['rounds'], 'ms_per_file_median': med, 'ms_min': lo, 'ms_max': hi, 'reps': reps,
                     'equals_host_model': bool(np.array_equal(d['coeffs'], raw['coeffs']))})
        print(json.dumps(rows[-1]), flush=True)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            json.dump(rows, f, indent=1)
            f.write('\n')
    return 0 if all(r['equals_host_model'] for r in rows) else 1


if __name__ == '__main__':
    sys.exit(main())
