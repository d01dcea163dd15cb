"""The reference pipeline on an arbitrary table and arbitrary symmetric taps.

oracle.cpu_ref.compress_reconstruct fixes the table to scale_quant_matrix(
JPEG_LUMA_Q50, quality) and the taps to gaussian_kernel3(0.75).  This is the
same chain (engines/pipeline.py:17-167), composed only from the oracle's stage
functions, with both as arguments; with the defaults it is the oracle's own
result (tests/test_params_cpu.py)."""
import numpy as np

from oracle import cpu_ref


def subsample(cb, cr, mode, prefilter, taps):
    """cpu_ref.subsample_chroma with the taps given (engines/color_space.py:27-53)."""
    if mode == '4:4:4':
        return cb.copy(), cr.copy()
    if prefilter:
        # cv2's SymmColumnFilter: k1 T[y] + k0 (T[y+1] + T[y-1]) -- defined for symmetric taps only
        assert taps[0] == taps[2], taps
        k = np.asarray(taps, np.float64)
        cb = cpu_ref.gaussian_blur3(cb, k)
        cr = cpu_ref.gaussian_blur3(cr, k)
    h, w = cb.shape
    oh = h // 2 if mode == '4:2:0' else h
    return cpu_ref.resize_area(cb, oh, w // 2), cpu_ref.resize_area(cr, oh, w // 2)


def planes(img, mode, prefilter, taps):
    """[Y, Cb, Cr] as the block stage receives them (fp64, not level-shifted)."""
    ycc = cpu_ref.rgb_to_ycbcr(img.astype(np.float64))
    cb, cr = subsample(ycc[:, :, 1], ycc[:, :, 2], mode, prefilter, taps)
    return [ycc[:, :, 0], cb, cr]


def dct_planes(img, mode, prefilter, taps, block_size=8):
    """Per plane (Y, Cb, Cr): the unquantised coefficients (n, B, B) of the padded
    plane, the padded shape and the plane's own shape; and the luma plane."""
    out = []
    pl = planes(img, mode, prefilter, taps)
    for ch in pl:
        padded, orig = cpu_ref.pad_to_multiple(ch, block_size)
        out.append((cpu_ref.encode_blocks(cpu_ref.split_blocks(padded, block_size)), padded.shape, orig))
    return out, pl[0]


def table_of(qtable, block_size=8):
    qm = np.asarray(qtable, np.float64).reshape(8, 8)
    return cpu_ref.quant_table16(qm) if block_size == 16 else qm


def compress_reconstruct(img, qtable, mode, prefilter, taps, block_size=8):
    """coeffs, reconstructed, hist, bitrate, error_map_y as cpu_ref.compress_reconstruct returns them."""
    assert taps[0] == taps[2], taps
    assert mode in cpu_ref.MODES and block_size in (8, 16)
    shape = img.shape[:2]
    B = block_size
    qm = table_of(qtable, B)
    dct, y = dct_planes(img, mode, prefilter, taps, B)
    parts, rec = [], []
    for c, padded_shape, orig in dct:
        qb = cpu_ref.quantize(c, qm)
        parts.append(qb.reshape(-1))
        r = cpu_ref.decode_blocks(cpu_ref.dequantize(qb, qm))
        rec.append(cpu_ref.merge_blocks(r, padded_shape)[:orig[0], :orig[1]])
    y_rec, cb_rec, cr_rec = rec
    if mode != '4:4:4':
        cb_rec, cr_rec = cpu_ref.upsample_chroma(cb_rec, cr_rec, shape)
    rgb_f = cpu_ref.ycbcr_to_rgb(np.stack([y_rec, cb_rec, cr_rec], axis=-1))
    all_q = np.concatenate(parts)
    return {'coeffs': all_q, 'reconstructed': np.clip(rgb_f, 0, 255).astype(np.uint8),
            'hist': np.histogram(all_q, bins=50, range=(-100, 100))[0],
            'bitrate': cpu_ref.estimate_bitrate_no_entropy(all_q, shape, B),
            'error_map_y': np.abs(y - y_rec)}
