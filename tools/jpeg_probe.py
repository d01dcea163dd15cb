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
rocprofv3 --kernel-trace --stats, which gives the per-kernel split)."""
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


def main():
    H, W = int(os.environ.get('HEIGHT', '1080')), int(os.environ.get('WIDTH', '1920'))
    reps = 1 if '--once' in sys.argv else int(os.environ.get('REPS', '30'))
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
