"""Shared cases of the table / taps tests (test_params_cpu.py, test_gpu_params.py).

The C ABI takes any integer table in [1, 255] and any symmetric finite taps
(include/jds.h); the values themselves choose kernels (the DC step routes the
inverse) and feed the certificates (the forward's per-coefficient bounds come
from Q and the taps, the full run's fixed |q Q| bound from the taps' signs and
sum).  TABLES and TAPS are the accepted values the tests run on, BAD_TAPS the
ones the library must refuse by name.  No GPU module is imported here."""
import numpy as np

from oracle import cpu_ref

# ITU-T T.81 Annex K.2, the chrominance table
CHROMA_Q50 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.float64).reshape(8, 8)


def _flat(v, at=None, val=None):
    q = np.full((8, 8), float(v))
    if at is not None:
        q[at] = float(val)
    return q


def _primes():
    """The odd primes 3 .. 251 cycled over the 64 entries: (float)(1 / Q) is never exact."""
    p = [n for n in range(3, 252) if all(n % d for d in range(2, int(n ** 0.5) + 1))]
    return np.array([p[i % len(p)] for i in range(64)], np.float64).reshape(8, 8)


def _tables():
    t = {}
    t['chroma50'] = cpu_ref.scale_quant_matrix(CHROMA_Q50, 50)
    t['chroma90'] = cpu_ref.scale_quant_matrix(CHROMA_Q50, 90)
    t['flat1'] = _flat(1)
    t['flat16'] = _flat(16)
    t['flat255'] = _flat(255)
    # both sides of the inverse's routing threshold (DC step <= 60), with AC
    # steps that contradict what the DC step suggests
    t['dc60_ac255'] = _flat(255, (0, 0), 60)
    t['dc61_ac1'] = _flat(1, (0, 0), 61)
    t['luma50_T'] = cpu_ref.scale_quant_matrix(cpu_ref.JPEG_LUMA_Q50, 50).T.copy()
    t['one_fine'] = _flat(255, (3, 5), 1)
    t['one_coarse'] = _flat(1, (0, 1), 255)
    t['primes'] = _primes()
    t['pow2'] = 2.0 ** ((np.arange(8)[:, None] + np.arange(8)[None, :]) % 8)
    t['rand_a'] = np.random.default_rng(2101).integers(1, 256, (8, 8)).astype(np.float64)
    t['rand_b'] = np.random.default_rng(2102).integers(1, 256, (8, 8)).astype(np.float64)
    for name, q in t.items():
        assert q.shape == (8, 8) and q.dtype == np.float64, name
        assert (q >= 1).all() and (q <= 255).all() and (q == np.floor(q)).all(), name
    return t


TABLES = _tables()

# symmetric taps: accepted
TAPS = {
    'gauss075': cpu_ref.gaussian_kernel3(0.75),
    'gauss05': cpu_ref.gaussian_kernel3(0.5),
    'gauss2': cpu_ref.gaussian_kernel3(2.0),
    'box': np.array([1.0 / 3.0] * 3),
    'identity': np.array([0.0, 1.0, 0.0]),
    'sub1': np.array([0.2, 0.5, 0.2]),
    'over1': np.array([0.4, 0.4, 0.4]),
    'sharp': np.array([-0.25, 1.5, -0.25]),
    'sharp2': np.array([-0.5, 2.0, -0.5]),
}

# refused whenever the prefilter runs
BAD_TAPS = {
    'asymmetric': np.array([0.5, 0.3, 0.2]),
    'one_ulp': np.array([0.25, 0.5, np.nextafter(0.25, 1.0)]),
    'nan': np.array([0.25, np.nan, 0.25]),
    'inf': np.array([np.inf, 0.5, np.inf]),
}


def apriori_ok(taps) -> bool:
    """The plan's premise for the fixed |q Q| <= 1152 bound of a prefiltered
    full run (csrc/jds_abi.hip): non-negative taps whose sum is at most 1."""
    k = np.asarray(taps, np.float64)
    return bool((k >= 0).all() and (k[0] + k[1] + k[2]) <= 1.0 + 2.0 ** -40)


def _basis_sign(u, v, scale):
    """255 where basis function (u, v) of the 8x8 DCT is positive, else 0, each
    sample `scale` pixels wide (2: the pattern a subsampled chroma block sees)."""
    n = np.arange(8)
    cu = np.cos((2 * n + 1) * u * np.pi / 16)
    cv = np.cos((2 * n + 1) * v * np.pi / 16)
    p = (np.outer(cu, cv) > 0).astype(np.uint8) * 255
    return np.kron(p, np.ones((scale, scale), np.uint8))


def _bound_inputs(h, w):
    """Frames that drive |c| to its largest: pure 0 / 255 channels, 8x8
    checkerboards, basis sign patterns in luma (gray) and in Cb / Cr (blue
    against yellow, red against cyan), uniform noise."""
    out = []
    for rgb in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)):
        out.append(np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy())
    yy, xx = np.mgrid[0:h, 0:w]
    for cell in (8, 16):
        m = (((yy // cell) + (xx // cell)) % 2).astype(np.uint8) * 255
        out.append(np.stack([m, m, m], axis=-1))
        out.append(np.stack([255 - m, 255 - m, m], axis=-1))
    for u, v in ((0, 0), (1, 1), (7, 7), (0, 7)):
        for scale in (1, 2):
            p = _basis_sign(u, v, scale)
            p = np.tile(p, (-(-h // p.shape[0]), -(-w // p.shape[1])))[:h, :w]
            out.append(np.stack([p, p, p], axis=-1))              # luma
            out.append(np.stack([255 - p, 255 - p, p], axis=-1))  # Cb
            out.append(np.stack([p, 255 - p, 255 - p], axis=-1))  # Cr
    out.append(cpu_ref.random_image(h, w, 1400))
    out.append((np.random.default_rng(1401).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8))
    return np.stack(out)


def sign_frames(h, w):
    """The blue/yellow (Cb) and red/cyan (Cr) sign patterns of _bound_inputs at
    chroma scale: (7, 7), the pattern a sharpening prefilter amplifies most."""
    p = _basis_sign(7, 7, 2)
    p = np.tile(p, (-(-h // p.shape[0]), -(-w // p.shape[1])))[:h, :w]
    return [np.stack([255 - p, 255 - p, p], axis=-1), np.stack([p, 255 - p, 255 - p], axis=-1)]
