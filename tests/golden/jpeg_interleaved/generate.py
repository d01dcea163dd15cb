"""Writes this directory's fixtures: Pillow-made baseline JPEGs (one interleaved
scan, two quantisation tables), each file's expected cropped coefficients from
tests/interleaved_ref.py's decoder, and manifest.json.  Needs Pillow; the tests
read the committed files and do not.  Run from the repository root:

    python tests/golden/jpeg_interleaved/generate.py
"""
import io
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import interleaved_ref as ir  # noqa: E402

SUB = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
# (name, H, W, mode, content, Pillow save arguments)
CASES = [
    ('p17x23_420', 17, 23, '4:2:0', 'noise', {'quality': 50}),
    ('p24x40_420', 24, 40, '4:2:0', 'noise', {'quality': 50}),
    ('p33x35_422', 33, 35, '4:2:2', 'noise', {'quality': 50}),
    ('p9x9_444', 9, 9, '4:4:4', 'noise', {'quality': 50}),
    ('p16x16_420_gray', 16, 16, '4:2:0', 'gray', {'quality': 50}),
    ('p40x72_420_rst2', 40, 72, '4:2:0', 'noise', {'quality': 50, 'restart_marker_blocks': 2}),
    ('p48x48_420_opt_rstrow', 48, 48, '4:2:0', 'noise', {'quality': 50, 'optimize': True, 'restart_marker_rows': 1}),
    ('p31x45_420_q95_opt', 31, 45, '4:2:0', 'noise', {'quality': 95, 'optimize': True}),
]
SEED = 20240611


def image(i, H, W, content):
    if content == 'gray':
        return np.full((H, W, 3), 128, np.uint8)
    return np.random.default_rng(SEED + i).integers(0, 256, (H, W, 3), dtype=np.uint8)


def main():
    manifest = {'pillow': PIL.__version__, 'seed': SEED, 'files': {}}
    for i, (name, H, W, mode, content, args) in enumerate(CASES):
        buf = io.BytesIO()
        Image.fromarray(image(i, H, W, content)).save(buf, 'JPEG', subsampling=SUB[mode], **args)
        data = buf.getvalue()
        d = ir.decode(data)
        assert (d['H'], d['W'], d['mode']) == (H, W, mode) and d['interleaved']
        assert ir.entropy_segment(d['padded'], H, W, mode, d['huff'], d['scan_tables'], d['ri']) == d['segment']
        kept = sum(r * c for r, c in d['grids'])
        total = sum(p.shape[0] * p.shape[1] for p in d['padded'])
        open(os.path.join(HERE, name + '.jpg'), 'wb').write(data)
        np.save(os.path.join(HERE, name + '.npy'), d['planar'])
        manifest['files'][name] = {
            'H': H, 'W': W, 'mode': mode, 'content': content, 'seed': SEED + i, 'args': args, 'bytes': len(data),
            'grids': [list(g) for g in d['grids']], 'mcu': list(d['mcu']), 'padded_blocks': total - kept,
            'restart_interval': d['ri'], 'tq': d['tq'],
            'max_code_length': max(max(l + 1 for l, n in enumerate(b) if n) for b, _ in d['huff'].values())}
    with open(os.path.join(HERE, 'manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
