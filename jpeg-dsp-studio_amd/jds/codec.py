"""Host-side calls into libjds.so for the drop-in engines.* / utils.metrics API.

Everything here marshals NumPy arrays across the C-ABI; all per-sample
arithmetic happens in the HIP kernels.  Only parameter setup is done on the
host: the quantisation table (engines/quantizer.py:7-19, computed by the caller
with the reference's NumPy expression) and the 3 prefilter taps below.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import numpy as np

from . import _abi
from ._abi import check, lease, lib, make_params


def gaussian_kernel3(sigma: float = 0.75) -> np.ndarray:
    """Taps of cv2.GaussianBlur(ksize=(3,3), sigmaX=sigma) for CV_64F
    (engines/color_space.py:39-40): OpenCV's getGaussianKernelBitExact for n=3:
    t = exp(4 * (-0.125 / sigma^2)), k = [t, 1, t] / (2t + 1) computed as t * (1/sum)."""
    scale2x = -0.125 / (float(sigma) * float(sigma))
    t = math.exp(4.0 * scale2x)
    mul1 = 1.0 / ((t * 2.0) + 1.0)
    e = t * mul1
    return np.array([e, mul1, e], dtype=np.float64)


def _taps(gauss) -> np.ndarray:
    """The prefilter's taps as jds_params.gauss takes them (None: the reference's)."""
    if gauss is None:
        return gaussian_kernel3(0.75)
    g = np.ascontiguousarray(gauss, dtype=np.float64).reshape(-1)
    if g.size != 3:
        raise ValueError(f'the prefilter takes three taps, got {g.size}')
    return g


def _u8_image(image: np.ndarray) -> np.ndarray:
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('Input images must have the same dimensions.' if a.ndim == 3 else
                         f'compress_reconstruct expects an HxWx3 RGB image, got shape {a.shape}')
    if a.dtype != np.uint8:
        if not np.issubdtype(a.dtype, np.integer) or a.min(initial=0) < 0 or a.max(initial=0) > 255:
            raise ValueError(f'the MI355X path takes uint8 RGB images (got {a.dtype})')
        a = a.astype(np.uint8)
    return np.ascontiguousarray(a)


def compress_reconstruct_raw(image: np.ndarray, quality: int, qtable: np.ndarray, mode: str, prefilter: bool,
                             block_size: int = 8, selected_block_idx: Tuple[int, int] = (0, 0),
                             maps: bool = True, device: int = 0, gauss=None) -> Dict[str, object]:
    """One jds_compress_reconstruct call (include/jds.h): returns the raw outputs.
    gauss: the prefilter's three taps (None: gaussian_kernel3(0.75), the reference's);
    symmetric and finite wherever the prefilter runs."""
    img = _u8_image(image)
    H, W = img.shape[:2]
    p = make_params(quality, qtable, mode, prefilter, _taps(gauss), block_size)
    geo = _abi.geometry(p, H, W)
    out = np.empty_like(img)
    coeffs = np.empty(geo.coeffs_per_frame, dtype=np.int16)
    st = _abi.FrameStats()
    ey = np.empty((H, W), np.float64) if maps else None
    er = np.empty((H, W), np.float64) if maps else None
    sel = _abi.SelectedBlock()
    sel_ok = C.c_int32(0)
    with lease(device) as ctx:
        check(lib().jds_compress_reconstruct(
            ctx.handle, C.byref(p), img.ctypes.data, H, W, out.ctypes.data, coeffs.ctypes.data, C.byref(st),
            ey.ctypes.data if maps else None, er.ctypes.data if maps else None,
            int(selected_block_idx[0]), int(selected_block_idx[1]), C.byref(sel), C.byref(sel_ok)))
    res: Dict[str, object] = {'reconstructed': out, 'coeffs': coeffs, 'stats': st, 'geometry': geo,
                              'error_map_y': ey, 'error_map_rgb': er, 'selected': None}
    if sel_ok.value:
        def arr(field, dt=np.float64):
            return np.ctypeslib.as_array(getattr(sel, field)).astype(dt).reshape(8, 8)
        res['selected'] = {'original': arr('original'), 'shifted': arr('shifted'), 'dct': arr('dct'),
                           'quantized': arr('quantized', np.int16), 'dequantized': arr('dequantized'),
                           'reconstructed': arr('reconstructed')}
    return res


def decompress_jfif(data, device: int = 0, with_info: bool = False):
    """jds_decompress_jfif: a baseline JFIF of the profile this library writes -> the HxWx3
    uint8 image this codec reconstructs from its coefficients (the bytes
    compress_reconstruct_raw returned for the frame that made the file);
    with_info: (image, {'coeffs', 'H', 'W', 'mode', 'qtable', 'rounds'})."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    info = _abi.JfifInfo()
    check(lib().jds_jfif_parse(p, n, C.byref(info)))
    H, W = int(info.H), int(info.W)
    img = np.empty((H, W, 3), np.uint8)
    cf = np.empty(int(info.coeffs_needed), np.int16)
    with lease(device) as ctx:
        check(lib().jds_decompress_jfif(ctx.handle, p, n, img.ctypes.data, img.size, cf.ctypes.data, C.byref(info)))
    if not with_info:
        return img
    d = entropy._info_dict(info)
    return img, {'coeffs': cf, 'H': H, 'W': W, 'mode': d['mode'], 'qtable': d['qtable'], 'rounds': int(info.rounds)}


def staged_inverse(coeffs: np.ndarray, H: int, W: int, mode: str, qtables, grids) -> np.ndarray:
    """The reference's inverse stages on planar coefficients (Y, Cb, Cr; each component's blocks
    in raster order of its (rows, cols) grid) with one table per component, through the
    per-stage calls only: dequantise, decode_block, merge and crop to the component's T.81
    plane size, bilinear chroma upsampling unless 4:4:4, YCbCr -> RGB, clip, truncate."""
    hmax, vmax = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2), 'gray': (1, 1)}[mode]
    cf = np.asarray(coeffs, np.int16).reshape(-1, 8, 8)
    planes, b0 = [], 0
    if mode == 'gray':   # one plane; each channel is its byte (the colour expressions at Cb = Cr = 128 give Y)
        grids = list(grids)[:1]
    for c, (gr, gc) in enumerate(grids):
        hs, vs = (hmax, vmax) if c == 0 else (1, 1)
        ph, pw = -(-H * vs // vmax), -(-W * hs // hmax)
        blk = stage_block(stage_quant(cf[b0:b0 + gr * gc], np.asarray(qtables[c], np.float64).reshape(8, 8), True), 3)
        b0 += gr * gc
        plane = blk.reshape(gr, gc, 8, 8).transpose(0, 2, 1, 3).reshape(8 * gr, 8 * gc)[:ph, :pw]
        planes.append(plane if (ph, pw) == (H, W) else stage_resize(plane, H, W, nearest=False))
    if mode == 'gray':
        return np.repeat(np.clip(planes[0], 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)
    rgb = stage_rgb_ycbcr(np.stack(planes, axis=-1), inverse=True)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def decompress_jpeg(data, device: int = 0, with_info: bool = False, staged: bool | None = None):
    """A baseline JPEG with one interleaved scan or three non-interleaved ones -> the HxWx3
    uint8 image.  Plan route (jds_decompress_jpeg, as decompress_jfif) when one quantisation
    table serves all components and the block grids are the reference's; otherwise (a grayscale
    file always), or with
    staged=True, the staged route: entropy.decode_jpeg, then staged_inverse with the file's own
    tables (not a throughput path).  with_info: (image, decode_jpeg's dict plus 'route')."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_parse(p, n, C.byref(info)))
    plan_ok = bool(info.single_table) and bool(info.reference_grid)
    if staged is False and not plan_ok:
        raise ValueError('the plan route needs one quantisation table and the reference block grids')
    if plan_ok and not staged:
        H, W = int(info.H), int(info.W)
        img = np.empty((H, W, 3), np.uint8)
        cf = np.empty(int(info.coeffs_needed), np.int16)
        with lease(device) as ctx:
            check(lib().jds_decompress_jpeg(ctx.handle, p, n, img.ctypes.data, img.size, cf.ctypes.data,
                                            C.byref(info)))
        d = entropy._jpeg_dict(info)
        d.update(coeffs=cf, rounds=int(info.rounds), route='plan')
    else:
        d = entropy.decode_jpeg(a, device)
        d['route'] = 'staged'
        img = staged_inverse(d['coeffs'], d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
    return (img, d) if with_info else img


def jpeg_inverse_info() -> Tuple[int, int]:
    """(tile_h, tile_w): the output pixels one workgroup of the fused inverse produces."""
    th, tw = C.c_int32(0), C.c_int32(0)
    check(lib().jds_jpeg_inverse_info(C.byref(th), C.byref(tw)))
    return int(th.value), int(tw.value)


def _jpeg_info_struct(H: int, W: int, mode: str, qtables, grids) -> _abi.JpegInfo:
    """The fields the fused inverse reads, from parse_jpeg's / decode_jpeg's terms."""
    info = _abi.JpegInfo()
    info.H, info.W, info.subsampling = int(H), int(W), _abi.JPEG_MODE_CODES[mode]
    q = np.ascontiguousarray(qtables, np.float64).reshape(3, 64)
    for c, (gr, gc) in enumerate(grids):
        info.grid_rows[c], info.grid_cols[c] = int(gr), int(gc)
        for i in range(64):
            info.qtable[c][i] = q[c, i]
    info.coeffs_needed = 64 * sum(int(gr) * int(gc) for gr, gc in grids)
    return info


def jpeg_inverse_dev(info: dict, coeffs_ptr: int, rgb_ptr: int, stream=None, device: int = 0) -> None:
    """jds_jpeg_inverse_dev: coefficients on the device (decode_jpeg's layout, int16) -> H*W*3
    RGB bytes on the device, one asynchronous launch on `stream` (a HIP stream handle; None: the
    null stream).  info: what entropy.parse_jpeg or decode_jpeg returned for the file."""
    st = _jpeg_info_struct(info['H'], info['W'], info['mode'], info['qtables'], info['grids'])
    with lease(device) as ctx:
        check(lib().jds_jpeg_inverse_dev(ctx.handle, C.byref(st), C.c_void_p(int(coeffs_ptr)),
                                         C.c_void_p(int(rgb_ptr)), C.c_void_p(int(stream or 0))))


def host_jpeg_inverse(coeffs: np.ndarray, H: int, W: int, mode: str, qtables, grids) -> np.ndarray:
    """Test aid (jds_selftest_jpeg_inverse): the fused inverse's tile core in a host tile loop,
    staged_inverse's arguments.  No GPU."""
    st = _jpeg_info_struct(H, W, mode, qtables, grids)
    cf = np.ascontiguousarray(coeffs, np.int16).reshape(-1)
    if cf.size != int(st.coeffs_needed):
        raise ValueError(f'expected {int(st.coeffs_needed)} coefficients, got {cf.size}')
    img = np.empty((int(H), int(W), 3), np.uint8)
    check(lib().jds_selftest_jpeg_inverse(C.byref(st), cf.ctypes.data, img.ctypes.data))
    return img


def jpeg_scaled_size(H: int, W: int, scale_denom: int = 1) -> Tuple[int, int]:
    """jds_jpeg_scaled_size: (ceil(H / scale_denom), ceil(W / scale_denom)), the image an H x W
    file decodes to at scale_denom 1, 2, 4 or 8."""
    d = _abi.scale_denom_arg(scale_denom)
    oh, ow = C.c_int64(0), C.c_int64(0)
    check(lib().jds_jpeg_scaled_size(int(H), int(W), d, C.byref(oh), C.byref(ow)))
    return int(oh.value), int(ow.value)


def draft_denom(H: int, W: int, size) -> int:
    """The denominator Pillow's Image.draft(mode, size) chooses for an H x W file and a requested
    size (width, height): the largest of 8, 4, 2, 1 that is at most min(W // size[0],
    H // size[1]), so the scaled image still covers the request on both axes."""
    rw, rh = int(size[0]), int(size[1])
    if rw < 1 or rh < 1:
        raise ValueError(f'bad requested size {size!r}')
    scale = min(int(W) // rw, int(H) // rh)
    return 8 if scale >= 8 else 4 if scale >= 4 else 2 if scale >= 2 else 1


def jpeg_render_dev(info: dict, coeffs_ptr: int, rgb_ptr: int, render: str = 'libjpeg', stream=None,
                    device: int = 0, scale_denom: int = 1) -> None:
    """jds_jpeg_render_dev: jpeg_inverse_dev with the rendering chosen -- 'reference' (the launch
    jpeg_inverse_dev makes) or 'libjpeg' (k_jpeg_ljt: libjpeg's default decode byte for byte,
    DESIGN.md "libjpeg rendering").  scale_denom 2, 4 or 8 (render='libjpeg' only):
    jds_jpeg_render_scaled_dev, k_jpeg_ljs; rgb_ptr then holds jpeg_scaled_size's image."""
    code = _abi.render_code(render)
    d = _abi.scale_denom_arg(scale_denom, render)
    st = _jpeg_info_struct(info['H'], info['W'], info['mode'], info['qtables'], info['grids'])
    with lease(device) as ctx:
        if d == 1:
            check(lib().jds_jpeg_render_dev(ctx.handle, C.byref(st), C.c_void_p(int(coeffs_ptr)),
                                            C.c_void_p(int(rgb_ptr)), C.c_void_p(int(stream or 0)), code))
        else:
            check(lib().jds_jpeg_render_scaled_dev(ctx.handle, C.byref(st), C.c_void_p(int(coeffs_ptr)),
                                                   C.c_void_p(int(rgb_ptr)), C.c_void_p(int(stream or 0)), code, d))


def host_jpeg_render(coeffs: np.ndarray, H: int, W: int, mode: str, qtables, grids, render: str = 'libjpeg',
                     scale_denom: int = 1) -> np.ndarray:
    """Test aid (jds_selftest_jpeg_render): host_jpeg_inverse with the rendering chosen; 'libjpeg'
    runs k_jpeg_ljt's tile core in a host tile loop, with scale_denom 2, 4 or 8 k_jpeg_ljs's
    (jds_selftest_jpeg_render_scaled).  No GPU."""
    code = _abi.render_code(render)
    d = _abi.scale_denom_arg(scale_denom, render)
    st = _jpeg_info_struct(H, W, mode, qtables, grids)
    cf = np.ascontiguousarray(coeffs, np.int16).reshape(-1)
    if cf.size != int(st.coeffs_needed):
        raise ValueError(f'expected {int(st.coeffs_needed)} coefficients, got {cf.size}')
    if d != 1:
        img = np.empty((-(-int(H) // d), -(-int(W) // d), 3), np.uint8)
        check(lib().jds_selftest_jpeg_render_scaled(C.byref(st), cf.ctypes.data, img.ctypes.data, code, d))
        return img
    img = np.empty((int(H), int(W), 3), np.uint8)
    check(lib().jds_selftest_jpeg_render(C.byref(st), cf.ctypes.data, img.ctypes.data, code))
    return img


def jpeg_to_rgb(data, device: int = 0, with_info: bool = False, out=None, render: str = 'reference',
                scale_denom: int = 1):
    """jds_jpeg_to_rgb: any baseline JPEG parse_jpeg accepts -> the HxWx3 uint8 image, by the
    entropy decode and one fused inverse launch (k_jpeg_inv) with the file's own tables and
    grids: byte for byte decompress_jpeg(staged=True)'s image.  out: an object with data_ptr()
    (a contiguous uint8 torch tensor of shape (H, W, 3) on `device`): the image stays on the
    device, written there, and `out` is returned.  with_info: (image, decode_jpeg's dict plus
    'route': 'fused').  render='libjpeg': the same decode, rendered by k_jpeg_ljt to the bytes
    libjpeg's default decode gives (np.asarray(PIL.Image.open(f).convert('RGB')); DESIGN.md
    "libjpeg rendering").  scale_denom 2, 4 or 8 (render='libjpeg' only): libjpeg's reduced-size
    decode, PIL's Image.draft, byte for byte (k_jpeg_ljs; DESIGN.md "Scaled libjpeg rendering"):
    the image, and `out`, are jpeg_scaled_size(H, W, scale_denom) x 3; the info dict gains
    'scale_denom', 'out_H', 'out_W'."""
    from . import entropy
    code = _abi.render_code(render)
    d = _abi.scale_denom_arg(scale_denom, render)
    a, p, n = entropy._bytes_arg(data)
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_parse(p, n, C.byref(info)))
    fH, fW = int(info.H), int(info.W)
    H, W = -(-fH // d), -(-fW // d)
    if out is None:
        img = np.empty((H, W, 3), np.uint8)
        dst, on_dev = img.ctypes.data, 0
    else:
        if tuple(out.shape) != (H, W, 3) or not out.is_contiguous() or out.element_size() != 1:
            raise ValueError(f'out must be a contiguous uint8 ({H}, {W}, 3) device tensor')
        img, dst, on_dev = out, int(out.data_ptr()), 1
        _torch_settled(device)
    cf = np.empty(int(info.coeffs_needed), np.int16) if with_info else None
    with lease(device) as ctx:
        if d != 1:
            check(lib().jds_jpeg_to_rgb_scaled(ctx.handle, p, n, C.c_void_p(dst), H * W * 3, on_dev,
                                               cf.ctypes.data if with_info else None, C.byref(info), code, d))
        elif code == 0:
            check(lib().jds_jpeg_to_rgb(ctx.handle, p, n, C.c_void_p(dst), H * W * 3, on_dev,
                                        cf.ctypes.data if with_info else None, C.byref(info)))
        else:
            check(lib().jds_jpeg_to_rgb_render(ctx.handle, p, n, C.c_void_p(dst), H * W * 3, on_dev,
                                               cf.ctypes.data if with_info else None, C.byref(info), code))
    if not with_info:
        return img
    dd = entropy._jpeg_dict(info)
    dd.update(coeffs=cf, rounds=int(info.rounds), route='fused', scale_denom=d, out_H=H, out_W=W)
    return img, dd


def _batch_args(files):
    """(keep-alive arrays, pointer array, length array) of a sequence of bytes-like files; an
    empty one keeps its place with length 0 (the parser names it)."""
    keep = []
    for f in files:
        a = np.ascontiguousarray(f, np.uint8).reshape(-1) if isinstance(f, np.ndarray) else np.frombuffer(bytes(f), np.uint8)
        keep.append((a, a if a.size else np.zeros(1, np.uint8)))
    n = len(keep)
    ptrs = (C.c_void_p * max(n, 1))(*[k[1].ctypes.data for k in keep])
    lens = (C.c_int64 * max(n, 1))(*[int(k[0].size) for k in keep])
    return keep, ptrs, lens


def _batch_denoms(scale_denom, n: int, render=None):
    """(per-file denominators, the int32 array for the C call or None when all are 1)."""
    if not isinstance(scale_denom, (list, tuple, np.ndarray)):
        scale_denom = [_abi.scale_denom_arg(scale_denom, render)] * n
    dens = [_abi.scale_denom_arg(v, render) for v in _per_item(scale_denom, n, 'scale_denom')]
    if all(v == 1 for v in dens):
        return dens, None
    return dens, (C.c_int32 * max(n, 1))(*dens)


def _batch_item_dict(it, denom: int = 1) -> dict:
    from . import entropy
    ok = it.rc == 0
    return {'scale_denom': denom, 'out_H': -(-int(it.H) // denom) if it.H > 0 else 0,
            'out_W': -(-int(it.W) // denom) if it.H > 0 else 0, 'rc': int(it.rc), 'status': int(it.status), 'H': int(it.H), 'W': int(it.W),
            'mode': entropy._MODE_NAMES.get(int(it.subsampling)) if it.H > 0 else None,
            'interleaved': bool(it.interleaved), 'rgb_off': int(it.rgb_off) if ok else -1,
            'coef_off': int(it.coef_off) if ok else -1, 'coeffs_needed': int(it.coeffs_needed)}


def _batch_layout_call(ptrs, lens, n, items, rb, ce, dens_c):
    if dens_c is None:
        return lib().jds_jpeg_batch_layout(ptrs, lens, n, items, C.byref(rb), C.byref(ce))
    return lib().jds_jpeg_batch_layout_scaled(ptrs, lens, n, items, C.byref(rb), C.byref(ce), dens_c, None)


def jpeg_batch_layout(files, scale_denom=1):
    """jds_jpeg_batch_layout (host only): (per-file dicts, rgb_bytes, coef_entries) of a batch.
    A file's image is bytes [rgb_off, rgb_off + out_H*out_W*3) of the batch's output (rgb_off a
    multiple of 256), its coefficients entries [coef_off, coef_off + coeffs_needed); a file that
    does not parse has rc != 0 and takes no space.  scale_denom: 1, 2, 4 or 8, or one per file
    (jds_jpeg_batch_layout_scaled): the images are placed by their scaled sizes."""
    keep, ptrs, lens = _batch_args(files)
    n = len(keep)
    dens, dens_c = _batch_denoms(scale_denom, n)
    items = (_abi.JpegBatchItem * max(n, 1))()
    rb, ce = C.c_int64(0), C.c_int64(0)
    check(_batch_layout_call(ptrs, lens, n, items, rb, ce, dens_c))
    return [_batch_item_dict(items[i], dens[i]) for i in range(n)], int(rb.value), int(ce.value)


def _batch_first_error(items) -> str:
    msg = lib().jds_last_error().decode(errors='replace')
    for i, it in enumerate(items):
        if it['rc'] != 0:
            return msg or f'file {i}: error {it["rc"]}'
        if it['status'] != 0:
            return f'file {i}: defective scan data (status 0x{it["status"]:x})'
    return ''


def jpeg_batch_to_rgb(files, device: int = 0, out=None, with_info: bool = False, errors: str = 'raise', ctx=None,
                      render: str = 'reference', scale_denom=1):
    """jds_jpeg_batch_to_rgb: a sequence of baseline JPEGs (bytes-likes; any mix of sizes,
    subsampling modes, tables, restart intervals and scan forms) -> their images, decoded in one
    set of launches; each image is byte for byte jpeg_to_rgb's.  out=None: a list of HxWx3 uint8
    arrays; out='device': torch.uint8 tensors, views into one allocation on `device`; out a 1-D
    uint8 device tensor of at least jpeg_batch_layout's rgb_bytes: views into that.  A file that
    does not parse, or whose scan data are defective, does not stop the others: errors='raise'
    raises ValueError naming the first such index after the batch has run, errors='return' puts
    None in its place.  with_info: (images, {'items': per-file dicts, 'rounds': the batch's
    propagation rounds, 'rgb_bytes', 'coef_entries'}).  ctx: a caller-owned Context of that device
    (e.g. a profiled one) instead of a pooled one.  render='libjpeg': every image rendered as
    jpeg_to_rgb(render='libjpeg') does (k_jpeg_ljt_batch), the same layout and error contract.
    scale_denom: 1, 2, 4 or 8, or one per file (render='libjpeg' for any other than 1): each
    image is jpeg_to_rgb(scale_denom=...)'s, out_H x out_W x 3, placed by that size
    (k_jpeg_ljs_batch, one launch per mode and denominator present)."""
    return _batch_to_rgb(files, device, out, with_info, errors, ctx, render, scale_denom)


def _batch_to_rgb(files, device, out, with_info, errors, ctx, render, scale_denom, progressive=False):
    """jpeg_batch_to_rgb, and with `progressive` pjpeg_batch_to_rgb: the same buffers, items and
    errors around the layout call and the run call of either kind of file."""
    if errors not in ('raise', 'return'):
        raise ValueError("errors must be 'raise' or 'return'")
    code = _abi.render_code(render)
    keep, ptrs, lens = _batch_args(files)
    n = len(keep)
    dens, dens_c = _batch_denoms(scale_denom, n, render)
    items = (_abi.JpegBatchItem * max(n, 1))()
    if out is None or isinstance(out, str):
        # the output is sized here, from the layout; a caller's buffer is checked by the call itself
        rb, ce = C.c_int64(0), C.c_int64(0)
        if progressive:
            check(lib().jds_pjpeg_batch_layout(ptrs, lens, n, items, C.byref(rb), C.byref(ce), dens_c, None))
        else:
            check(_batch_layout_call(ptrs, lens, n, items, rb, ce, dens_c))
        cap = int(rb.value)
    if out is None:
        buf = np.empty(max(cap, 1), np.uint8)
        dst, on_dev = buf.ctypes.data, 0
    else:
        if isinstance(out, str):
            if out != 'device':
                raise ValueError("out must be None, 'device' or a 1-D uint8 device tensor")
            import torch
            buf = torch.empty(max(cap, 1), dtype=torch.uint8, device=f'cuda:{device}')
        else:
            buf = out
            if buf.dim() != 1 or buf.element_size() != 1 or not buf.is_contiguous():
                raise ValueError('out must be a contiguous 1-D uint8 device tensor')
            cap = int(buf.numel())
        dst, on_dev = int(buf.data_ptr()), 1
        _torch_settled(device)
    rounds = C.c_uint32(0)

    def run(c):
        if progressive:
            return lib().jds_pjpeg_batch_to_rgb(c.handle, ptrs, lens, n, C.c_void_p(dst), cap, on_dev, code, dens_c, items,
                                                None, None)
        if dens_c is not None:
            return lib().jds_jpeg_batch_to_rgb_scaled(c.handle, ptrs, lens, n, C.c_void_p(dst), cap, on_dev, None,
                                                      items, C.byref(rounds), code, dens_c, None)
        if code == 0:
            return lib().jds_jpeg_batch_to_rgb(c.handle, ptrs, lens, n, C.c_void_p(dst), cap, on_dev, None, items,
                                               C.byref(rounds))
        return lib().jds_jpeg_batch_to_rgb_render(c.handle, ptrs, lens, n, C.c_void_p(dst), cap, on_dev, None, items,
                                                  C.byref(rounds), code)
    if ctx is not None:
        check(run(ctx))
    else:
        with lease(device) as c:
            check(run(c))
    info = [_batch_item_dict(items[i], dens[i]) for i in range(n)]
    first = _batch_first_error(info)
    if first and errors == 'raise':
        raise ValueError(first)
    imgs = []
    for it in info:
        if it['rc'] != 0 or it['status'] != 0:
            imgs.append(None)
            continue
        o, sz = it['rgb_off'], it['out_H'] * it['out_W'] * 3
        imgs.append(buf[o:o + sz].reshape(it['out_H'], it['out_W'], 3))
    if not with_info:
        return imgs
    ok = [it for it in info if it['rc'] == 0]
    d = {'items': info, 'rgb_bytes': sum(-(-it['out_H'] * it['out_W'] * 3 // 256) * 256 for it in ok),
         'coef_entries': sum(it['coeffs_needed'] for it in ok)}
    if not progressive:
        d['rounds'] = int(rounds.value)     # (the chains of a progressive file have no propagation rounds)
    return imgs, d


def host_jpeg_batch(files, subseq_bits: int = 1024, render: str = 'reference', scale_denom=1):
    """Test aid (jds_selftest_jpeg_batch): the batch's layout, the host decode model per file and
    the host model of the batch inverse.  -> (rgb buffer, coefficient buffer, per-file dicts).  No GPU.
    render='libjpeg': jds_selftest_jpeg_batch_render with k_jpeg_ljt_batch's host model;
    scale_denom (an int or one per file): jds_selftest_jpeg_batch_render_scaled, k_jpeg_ljs_batch's."""
    code = _abi.render_code(render)
    keep, ptrs, lens = _batch_args(files)
    n = len(keep)
    dens, dens_c = _batch_denoms(scale_denom, n, render)
    items = (_abi.JpegBatchItem * max(n, 1))()
    rb, ce = C.c_int64(0), C.c_int64(0)
    check(_batch_layout_call(ptrs, lens, n, items, rb, ce, dens_c))
    rgb = np.full(max(int(rb.value), 1), 0xA5, np.uint8)
    cf = np.zeros(max(int(ce.value), 1), np.int16)
    if dens_c is not None:
        check(lib().jds_selftest_jpeg_batch_render_scaled(ptrs, lens, n, int(subseq_bits), rgb.ctypes.data,
                                                          int(rb.value), cf.ctypes.data, items, code, dens_c, None))
    elif code == 0:
        check(lib().jds_selftest_jpeg_batch(ptrs, lens, n, int(subseq_bits), rgb.ctypes.data, int(rb.value),
                                            cf.ctypes.data, items))
    else:
        check(lib().jds_selftest_jpeg_batch_render(ptrs, lens, n, int(subseq_bits), rgb.ctypes.data, int(rb.value),
                                                   cf.ctypes.data, items, code))
    return rgb[:int(rb.value)], cf[:int(ce.value)], [_batch_item_dict(items[i], dens[i]) for i in range(n)]


def jpeg_transcode(data, optimize: bool = True, device: int = 0, with_info: bool = False):
    """jds_jpeg_transcode: any baseline JPEG parse_jpeg accepts -> the same coefficients as one
    interleaved scan behind the file's own header segments (APPn, COM, DQT, SOF0 verbatim), with
    the file's own optimised Huffman tables (optimize=True: what `jpegtran -optimize` writes) or
    the Annex K ones.  Decode and write run on the device; no pixel and no coefficient changes
    (DESIGN.md "Transcode").  ValueError for a file the parser rejects, defective scan data, or a
    block baseline JPEG cannot code ("not baseline-codable").  with_info: (bytes, parse_jpeg's
    dict of the input plus 'rounds')."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    info = _abi.JpegInfo()
    with lease(device) as ctx:
        out = entropy._grown(lambda o, cap, m: lib().jds_jpeg_transcode(
            ctx.handle, p, n, int(bool(optimize)), o.ctypes.data, cap, C.byref(m), C.byref(info)),
            n + n // 4 + 4096)
    if not with_info:
        return out
    d = entropy._jpeg_dict(info)
    d['rounds'] = int(info.rounds)
    return out, d


def _transcode_item_dict(it) -> dict:
    from . import entropy
    return {'rc': int(it.rc), 'status': int(it.status), 'H': int(it.H), 'W': int(it.W),
            'mode': entropy._MODE_NAMES.get(int(it.subsampling)) if it.H > 0 else None,
            'interleaved': bool(it.interleaved), 'out_off': int(it.out_off), 'out_len': int(it.out_len)}


def jpeg_batch_transcode(files, optimize: bool = True, out=None, errors: str = 'raise', device: int = 0, ctx=None):
    """jds_jpeg_batch_transcode: a sequence of baseline JPEGs (any mix of sizes, modes, tables,
    restart intervals and scan forms) -> each one's jpeg_transcode output, by the batch decode's
    launches and one set of writer launches.  out=None: a list of bytes; out='device': torch.uint8
    tensors, views into one allocation on `device` (file i at a multiple of 256); out a 1-D uint8
    device tensor: views into that (ValueError naming the need when it is too small).  A file that
    does not parse, whose scan data are defective or that is not baseline-codable does not stop the
    others and no other file's bytes depend on it: errors='raise' raises ValueError naming the
    first such index after the batch has run; errors='items' returns (outputs with None in its
    place, per-file dicts: 'rc', 'status', 'out_off', 'out_len', ...).  ctx: a caller-owned Context
    (e.g. a profiled one) instead of a pooled one."""
    return _batch_transcode(files, optimize, out, errors, device, ctx, None)


def _batch_transcode(files, optimize, out, errors, device, ctx, ops, progressive=False):
    """jpeg_batch_transcode (ops None) and jpeg_batch_transform (ops: one JDS_XF_* code per file);
    progressive: pjpeg_batch_transcode (jds_pjpeg_batch_transcode, the same arguments)."""
    if errors not in ('raise', 'items'):
        raise ValueError("errors must be 'raise' or 'items'")
    keep, ptrs, lens = _batch_args(files)
    n = len(keep)
    if ops is not None:
        if len(ops) != n:
            raise ValueError(f'{len(ops)} operations for {n} files')
        ops_arr = (C.c_int32 * max(n, 1))(*ops)
    items = (_abi.JpegTranscodeItem * max(n, 1))()
    need = C.c_int64(0)
    own = out is None or isinstance(out, str)
    if isinstance(out, str) and out != 'device':
        raise ValueError("out must be None, 'device' or a 1-D uint8 device tensor")
    if not own and (out.dim() != 1 or out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError('out must be a contiguous 1-D uint8 device tensor')
    # a first guess from the inputs' sizes; the call reports the exact need when it is short
    cap = sum(-(-(int(k[0].size) * 5 // 4 + 4096) // 256) * 256 for k in keep) if own else int(out.numel())

    def run(c, buf, cap):
        dst, on_dev = (buf.ctypes.data, 0) if out is None else (int(buf.data_ptr()), 1)
        if ops is not None:
            return lib().jds_jpeg_batch_transform(c.handle, ptrs, lens, n, ops_arr, int(bool(optimize)),
                                                  C.c_void_p(dst), cap, on_dev, items, C.byref(need))
        call = lib().jds_pjpeg_batch_transcode if progressive else lib().jds_jpeg_batch_transcode
        return call(c.handle, ptrs, lens, n, int(bool(optimize)), C.c_void_p(dst), cap, on_dev, items, C.byref(need))

    def alloc(cap):
        if out is None:
            return np.empty(max(cap, 1), np.uint8)
        if isinstance(out, str):
            import torch
            return torch.empty(max(cap, 1), dtype=torch.uint8, device=f'cuda:{device}')
        return out

    def attempt(c):
        nonlocal cap
        buf = alloc(cap)
        rc = run(c, buf, cap)
        if rc == _abi.JDS_EINVAL and own and need.value > cap:
            cap = int(need.value)
            buf = alloc(cap)
            rc = run(c, buf, cap)
        check(rc)
        return buf

    if out is not None:
        _torch_settled(device)      # (once: torch queues nothing between here and a retry's allocation)
    if ctx is not None:
        buf = attempt(ctx)
    else:
        with lease(device) as c:
            buf = attempt(c)
    info = [_transcode_item_dict(items[i]) for i in range(n)]
    first = _batch_first_error(info)
    if first and errors == 'raise':
        raise ValueError(first)
    outs = []
    for it in info:
        if it['rc'] != 0 or it['status'] != 0:
            outs.append(None)
            continue
        v = buf[it['out_off']:it['out_off'] + it['out_len']]
        outs.append(v.tobytes() if out is None else v)
    return outs if errors == 'raise' else (outs, info)


def jpeg_transform_info(data, op: str = 'auto', trim: bool = False) -> dict:
    """jds_jpeg_transform_info (host only): what jpeg_transform would do to this file ->
    {'op': the operation, 'auto' resolved from the EXIF Orientation, 'H', 'W': the output's size}.
    ValueError for a file the parser rejects, a mirrored axis that is not whole MCUs without trim
    (it names the axis and the multiple), a transposing operation at 4:2:2, a trim that leaves
    nothing."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    op_out, H, W = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    check(lib().jds_jpeg_transform_info(p, n, _abi.xf_code(op, trim), C.byref(op_out), C.byref(H), C.byref(W)))
    return {'op': _abi.XF_NAMES[int(op_out.value)], 'H': int(H.value), 'W': int(W.value)}


def jpeg_transform(data, op: str = 'auto', trim: bool = False, optimize: bool = True, device: int = 0,
                   with_info: bool = False):
    """jds_jpeg_transform: jpeg_transcode with the image mirrored, transposed or rotated without
    re-compression (what `jpegtran -flip / -transpose / -rotate` does; DESIGN.md "Lossless
    transforms").  op: 'none', 'hflip', 'vflip', 'transpose', 'transverse', 'rot90' (clockwise),
    'rot180', 'rot270', or 'auto': the operation the EXIF Orientation tag asks for, the tag reset to 1
    (no usable tag: the plain transcode).  A mirrored axis must be whole MCUs: ValueError otherwise
    (`jpegtran -perfect`), or with trim=True the partial MCU column / row is dropped first
    (`jpegtran -trim`).  4:2:2 takes only 'hflip', 'vflip' and 'rot180'.  The coefficients never
    leave the device and change in sign only.  with_info: (bytes, parse_jpeg's dict of the input
    plus 'rounds' and 'transform': jpeg_transform_info's dict)."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    code = _abi.xf_code(op, trim)
    info = _abi.JpegInfo()
    with lease(device) as ctx:
        out = entropy._grown(lambda o, cap, m: lib().jds_jpeg_transform(
            ctx.handle, p, n, code, int(bool(optimize)), o.ctypes.data, cap, C.byref(m), C.byref(info)),
            n + n // 4 + 4096)
    if not with_info:
        return out
    d = entropy._jpeg_dict(info)
    d['rounds'] = int(info.rounds)
    d['transform'] = jpeg_transform_info(data, op, trim)
    return out, d


def jpeg_batch_transform(files, ops='auto', trim: bool = False, optimize: bool = True, out=None, errors: str = 'raise',
                         device: int = 0, ctx=None):
    """jds_jpeg_batch_transform: jpeg_batch_transcode with an operation per file -- each good
    file's bytes are jpeg_transform's.  ops: one name for all files or a list with one name per file
    (jpeg_transform's names); trim applies to all.  out, errors, ctx and the return shape as
    jpeg_batch_transcode; an item's 'H' and 'W' are the output's size, and a file whose operation is
    refused (a partial MCU on a mirrored axis without trim, a transposition at 4:2:2) is an item
    error that does not stop the others."""
    files = list(files)
    names = [ops] * len(files) if isinstance(ops, str) else list(ops)
    return _batch_transcode(files, optimize, out, errors, device, ctx, [_abi.xf_code(o, trim) for o in names])


# ----------------------------------------------------------- libjpeg encoding --
# (DESIGN.md "libjpeg encoding"; definition: tests/libjpeg_fwd_ref.py)

def is_progressive(data) -> bool:
    """True when the file's frame header is SOF2 (host only: a marker walk up to the first SOF or
    SOS; anything that is not a marker sequence from SOI is False).  Such a file goes through the
    pjpeg_* calls; the jpeg_* calls reject it by name."""
    b = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    if len(b) < 4 or b[0] != 0xFF or b[1] != 0xD8:
        return False
    p = 2
    while p + 4 <= len(b) and b[p] == 0xFF:
        m = b[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xC2:
            return True
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) or m in (0xDA, 0xD9):
            return False
        p += 2 + ((b[p + 2] << 8) | b[p + 3])
    return False


def pjpeg_to_rgb(data, out=None, render: str = 'libjpeg', scale_denom: int = 1, with_info: bool = False,
                 device: int = 0):
    """jds_pjpeg_to_rgb: a progressive JPEG parse_pjpeg accepts -> the image, by the chain decode
    (k_pjpeg_chains) and the rendering jpeg_to_rgb names: render='libjpeg' is byte for byte
    np.asarray(PIL.Image.open(f).convert('RGB')), with scale_denom 2, 4, 8 PIL's Image.draft;
    render='reference' is jpeg_to_rgb's image of the baseline file with the same coefficients.
    out, scale_denom and with_info (image, decode_pjpeg's dict) as jpeg_to_rgb's.  ValueError for
    a file the parser rejects (a baseline file: "not progressive"), for defective scan data and
    for a progression that stops short of Al = 0 ("incomplete progression": libjpeg smooths such
    a file; pjpeg_transcode takes it)."""
    from . import entropy
    code = _abi.render_code(render)
    d = _abi.scale_denom_arg(scale_denom, render)
    a, p, n = entropy._bytes_arg(data)
    info = _abi.PjpegInfo()
    check(lib().jds_pjpeg_parse(p, n, C.byref(info)))
    H, W = -(-int(info.frame.H) // d), -(-int(info.frame.W) // d)
    if out is None:
        img = np.empty((H, W, 3), np.uint8)
        dst, on_dev = img.ctypes.data, 0
    else:
        if tuple(out.shape) != (H, W, 3) or not out.is_contiguous() or out.element_size() != 1:
            raise ValueError(f'out must be a contiguous uint8 ({H}, {W}, 3) device tensor')
        img, dst, on_dev = out, int(out.data_ptr()), 1
        _torch_settled(device)
    cf = np.empty(int(info.frame.coeffs_needed), np.int16) if with_info else None
    with lease(device) as ctx:
        check(lib().jds_pjpeg_to_rgb(ctx.handle, p, n, C.c_void_p(dst), H * W * 3, on_dev, code, d,
                                     cf.ctypes.data if with_info else None, C.byref(info)))
    if not with_info:
        return img
    dd = entropy._pjpeg_dict(info)
    dd.update(coeffs=cf, route='chains', scale_denom=d, out_H=H, out_W=W)
    return img, dd


def pjpeg_batch_to_rgb(files, out='device', render: str = 'libjpeg', scale_denom=1, errors: str = 'raise',
                       with_info: bool = False, device: int = 0, ctx=None):
    """jds_pjpeg_batch_to_rgb: a sequence of progressive JPEGs -> their images, decoded by one
    k_pjpeg_chains launch over every file's chains and the batch render kernels jpeg_batch_to_rgb
    runs; each image is pjpeg_to_rgb's.  out, scale_denom, errors ('raise' / 'return'), with_info
    and ctx as jpeg_batch_to_rgb's, with its layout (images at multiples of 256) and its item
    contract: a baseline file ("not progressive"), an incomplete progression or defective scan
    data is that file's error and does not stop the others."""
    return _batch_to_rgb(files, device, out, with_info, errors, ctx, render, scale_denom, progressive=True)


def pjpeg_scan_times(ctx, files, took_part=None):
    """jds_pjpeg_scan_times: after a pjpeg_batch_* call on the profiled Context `ctx`
    (ctx.profile(True)), the walk time of every scan inside k_pjpeg_chains -> per file that took
    part (took_part: one flag per file, default all) a list of (scan index in file order,
    microseconds), None for the others."""
    from . import entropy
    n = C.c_int64(0)
    lib().jds_pjpeg_scan_times(ctx.handle, None, 0, C.byref(n))
    us = np.zeros(max(int(n.value), 1), np.float64)
    check(lib().jds_pjpeg_scan_times(ctx.handle, us.ctypes.data, int(n.value), C.byref(n)))
    out, k = [], 0
    for i, f in enumerate(files):
        if took_part is not None and not took_part[i]:
            out.append(None)
            continue
        scans = entropy.parse_pjpeg(f)['scans']
        order = [j for j, s in enumerate(scans) if s['ss'] == 0]
        for c in (1, 2, 3):
            order += [j for j, s in enumerate(scans) if s['ss'] and s['components'][0] == c]
        out.append([(j, float(us[k + m])) for m, j in enumerate(order)])
        k += len(order)
    if k != int(n.value):
        raise ValueError(f'{int(n.value)} scan times for {k} scans: the files are not the last call\'s')
    return out


def pjpeg_transcode(data, optimize: bool = True, device: int = 0, with_info: bool = False):
    """jds_pjpeg_transcode: a progressive JPEG -> the baseline file of the same coefficients
    (`jpegtran` from progressive to baseline): one interleaved scan behind the file's own APPn,
    COM and DQT segments and its frame header rewritten as SOF0, with optimised Huffman tables or
    the Annex K ones; every jpeg_* call reads the result.  A progression that stops short of
    Al = 0 transcodes as well: the coefficients are what the scans give.  ValueError as
    jpeg_transcode.  with_info: (bytes, parse_pjpeg's dict)."""
    from . import entropy
    a, p, n = entropy._bytes_arg(data)
    info = _abi.PjpegInfo()
    with lease(device) as ctx:
        out = entropy._grown(lambda o, cap, m: lib().jds_pjpeg_transcode(
            ctx.handle, p, n, int(bool(optimize)), o.ctypes.data, cap, C.byref(m), C.byref(info)),
            2 * n + 4096)
    return (out, entropy._pjpeg_dict(info)) if with_info else out


def pjpeg_batch_transcode(files, optimize: bool = True, out=None, errors: str = 'raise', device: int = 0, ctx=None):
    """jds_pjpeg_batch_transcode: a sequence of progressive JPEGs -> each one's pjpeg_transcode
    output, by one k_pjpeg_chains launch and one set of writer launches; arguments, packing (file
    i at a multiple of 256) and item contract of jpeg_batch_transcode.  out='device' feeds
    jpeg_batch_to_rgb, jpeg_batch_to_tensor and the transforms without leaving the device."""
    return _batch_transcode(files, optimize, out, errors, device, ctx, None, progressive=True)


def _ss_code(subsampling) -> int:
    if subsampling not in _abi.JPEG_MODE_CODES:
        raise ValueError(f'unknown subsampling {subsampling!r}: one of {", ".join(_abi.JPEG_MODE_CODES)}')
    return _abi.JPEG_MODE_CODES[subsampling]


def _quality_info(quality, code: int, H: int, W: int) -> _abi.JpegInfo:
    info = _abi.JpegInfo()
    check(lib().jds_jpeg_quality_info(int(quality), code, int(H), int(W), C.byref(info)))
    return info


def libjpeg_tables(quality: int) -> np.ndarray:
    """jpeg_set_quality(quality, force_baseline)'s tables: (2, 64) float64, luma and chroma,
    row-major.  ValueError for a quality outside 1..100."""
    info = _quality_info(quality, _abi.SS_444, 8, 8)
    return np.ctypeslib.as_array(info.qtable).astype(np.float64).reshape(3, 64)[:2].copy()


def _is_tensor(x) -> bool:
    return hasattr(x, 'data_ptr') and hasattr(x, 'is_contiguous')


def _image_arg(image, device: int = 0):
    """(keep-alive object, pointer, on_device, H, W, gray) of an HxWx3 or HxW uint8 NumPy array or
    contiguous torch tensor on GPU `device` (ValueError for one on another GPU)."""
    if _is_tensor(image):
        if image.is_cuda and image.device.index != int(device):
            raise ValueError(f'the image is on {image.device}, the call runs on device {int(device)}')
        shape = tuple(int(v) for v in image.shape)
        if image.element_size() != 1 or 'uint8' not in str(image.dtype):
            raise ValueError(f'images must be uint8 (got {image.dtype})')
        if not image.is_contiguous():
            raise ValueError('a device image must be a contiguous tensor')
        if not image.is_cuda:
            image = image.numpy()
    if not _is_tensor(image):
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise ValueError(f'images must be uint8 (got {a.dtype})')
        shape = a.shape
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)) or 0 in shape:
        raise ValueError(f'an image is HxWx3 or HxW (grayscale), got shape {tuple(shape)}')
    if _is_tensor(image):
        return image, int(image.data_ptr()), 1, shape[0], shape[1], len(shape) == 2
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data, 0, shape[0], shape[1], len(shape) == 2


def _torch_settled(device: int) -> None:
    """The context's stream does not wait for torch's: what torch has queued on its current stream
    ends first -- for a source tensor the work that produces it, for a destination tensor (the
    caller's, or one allocated here, whose block the caching allocator may have recycled from a
    tensor with work still queued) the work that would otherwise land after this call's."""
    import torch
    torch.cuda.current_stream(device).synchronize()


def _aligned_i16(n: int) -> np.ndarray:
    """n int16 entries starting at a 16-byte boundary."""
    raw = np.empty(2 * n + 16, np.uint8)
    o = (-raw.ctypes.data) % 16
    return raw[o:o + 2 * n].view(np.int16)


def host_rgb_forward(image, quality: int = 75, subsampling: str = '4:2:0'):
    """Test aid (jds_selftest_jpeg_forward): k_jpeg_fwd's tile core in a host tile loop -> (planar
    int16 coefficients in decode_jpeg's layout, info dict: 'H', 'W', 'mode', 'grids', 'qtables', 'tq',
    ... as parse_jpeg gives them) -- entropy.encode_jpeg's arguments.  A 2-D image is grayscale
    whatever `subsampling` says.  No GPU."""
    from . import entropy
    keep, p, on_dev, H, W, gray = _image_arg(image)
    if on_dev:
        raise ValueError('host_rgb_forward takes a host array')
    info = _quality_info(quality, _abi.SS_GRAY if gray else _ss_code(subsampling), H, W)
    cf = _aligned_i16(int(info.coeffs_needed))
    check(lib().jds_selftest_jpeg_forward(C.byref(info), p, cf.ctypes.data))
    return cf, entropy._jpeg_dict(info)


def rgb_forward_dev(info: dict, rgb_ptr: int, coeffs_ptr: int, stream=None, device: int = 0) -> None:
    """jds_jpeg_forward_dev: H*W*3 RGB bytes on the device (info['mode'] 'gray': H*W) -> the quantised
    coefficients libjpeg's compressor gives, in decode_jpeg's layout (int16, 16-byte aligned) on the
    device: one asynchronous launch of k_jpeg_fwd on `stream` (None: the null stream).  info: 'H',
    'W', 'mode', 'grids', 'qtables' (any integer tables in [1, 255]) as host_rgb_forward returns."""
    st = _jpeg_info_struct(info['H'], info['W'], info['mode'], info['qtables'], info['grids'])
    with lease(device) as ctx:
        check(lib().jds_jpeg_forward_dev(ctx.handle, C.byref(st), C.c_void_p(int(rgb_ptr)),
                                         C.c_void_p(int(coeffs_ptr)), C.c_void_p(int(stream or 0))))


def rgb_to_jpeg(image, quality: int = 75, subsampling: str = '4:2:0', optimize: bool = False, device: int = 0) -> bytes:
    """jds_rgb_to_jpeg: an HxWx3 (or HxW: grayscale) uint8 image -- a NumPy array or a contiguous
    torch tensor on `device` -- -> the baseline JPEG PIL.Image.save(quality=, subsampling=,
    optimize=) writes, byte for byte (DESIGN.md "libjpeg encoding"): k_jpeg_fwd, then the
    transcode's writer; the coefficients never leave the device.  ValueError for another dtype or
    shape, a non-contiguous tensor, a quality outside 1..100 or a side above 65535."""
    from . import entropy
    keep, p, on_dev, H, W, gray = _image_arg(image, device)
    code = _abi.SS_GRAY if gray else _ss_code(subsampling)
    if on_dev:
        _torch_settled(device)
    with lease(device) as ctx:
        return entropy._grown(lambda o, cap, m: lib().jds_rgb_to_jpeg(
            ctx.handle, C.c_void_p(p), on_dev, H, W, int(quality), code, int(bool(optimize)), o.ctypes.data, cap,
            C.byref(m)), H * W * (1 if gray else 3) + 4096)      # (noise at a high quality comes close to the image's own size)


def _per_item(v, n: int, what: str) -> list:
    if isinstance(v, (str, int, np.integer)):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f'{len(v)} {what} values for {n} images')
    return v


def rgb_batch_to_jpeg(images, quality=75, subsampling='4:2:0', optimize: bool = False, out=None, errors: str = 'raise',
                      device: int = 0, ctx=None):
    """jds_rgb_batch_to_jpeg: images -> each one's rgb_to_jpeg file, by one forward launch per
    subsampling mode present and one set of writer launches.  images: a sequence of uint8 arrays
    (HxWx3 or HxW), a sequence of contiguous device tensors (views into one allocation -- e.g.
    jpeg_batch_to_rgb(out='device')'s -- are passed by offset, anything else is gathered into one
    buffer first), or an NxHxWx3 device tensor; any mix of sizes.  quality, subsampling: one value or
    one per image (a 2-D image is grayscale whatever its entry says).  out, errors, ctx and the
    return shape as jpeg_batch_transcode: an image with a bad argument (quality 0, ...) does not stop
    the others and no other file's bytes depend on it."""
    if errors not in ('raise', 'items'):
        raise ValueError("errors must be 'raise' or 'items'")
    own = out is None or isinstance(out, str)
    if isinstance(out, str) and out != 'device':
        raise ValueError("out must be None, 'device' or a 1-D uint8 device tensor")
    if not own and (out.dim() != 1 or out.element_size() != 1 or not out.is_contiguous()):
        raise ValueError('out must be a contiguous 1-D uint8 device tensor')
    if _is_tensor(images):
        if images.dim() != 4:
            raise ValueError(f'a batch tensor is NxHxWx3, got shape {tuple(images.shape)}')
        if not images.is_contiguous():
            raise ValueError('a device image must be a contiguous tensor')
        images = [images[i] for i in range(int(images.shape[0]))]
    args = [_image_arg(im, device) for im in images]
    n = len(args)
    qs, modes = _per_item(quality, n, 'quality'), _per_item(subsampling, n, 'subsampling')
    codes = [_abi.SS_GRAY if a[5] else _ss_code(m) for a, m in zip(args, modes)]
    sizes = [a[3] * a[4] * (1 if a[5] else 3) for a in args]
    if n and all(a[2] for a in args):
        bases = {int(a[0].untyped_storage().data_ptr()) for a in args}
        if len(bases) == 1:                      # views into one allocation: by offset
            base, keep = bases.pop(), [a[0] for a in args]
            offs = [a[1] - base for a in args]
        else:                                    # gathered on the device
            import torch
            keep = torch.cat([a[0].reshape(-1) for a in args])
            base, offs = int(keep.data_ptr()), [0] + list(np.cumsum(sizes[:-1]))
        on_dev = 1
    else:                                        # host arrays (a device tensor among them comes to the host)
        offs = [0] + list(np.cumsum([-(-s // 256) * 256 for s in sizes[:-1]])) if n else []
        keep = np.zeros(max(sum(-(-s // 256) * 256 for s in sizes), 1), np.uint8)
        for a, o, s in zip(args, offs, sizes):
            src = a[0].cpu().numpy() if a[2] else a[0]
            keep[o:o + s] = src.reshape(-1)
        base, on_dev = keep.ctypes.data, 0
    if on_dev or out is not None:
        _torch_settled(device)
    items_in = (_abi.RgbItem * max(n, 1))()
    for i, (a, o) in enumerate(zip(args, offs)):
        items_in[i].rgb_off, items_in[i].H, items_in[i].W = int(o), a[3], a[4]
        items_in[i].quality, items_in[i].subsampling = int(qs[i]), codes[i]
    items = (_abi.JpegTranscodeItem * max(n, 1))()
    need = C.c_int64(0)
    cap = sum(-(-(s + 4096) // 256) * 256 for s in sizes) if own else int(out.numel())     # (rgb_to_jpeg's guess)

    def alloc(cap):
        if out is None:
            return np.empty(max(cap, 1), np.uint8)
        if isinstance(out, str):
            import torch
            return torch.empty(max(cap, 1), dtype=torch.uint8, device=f'cuda:{device}')
        return out

    def run(c, buf, cap):
        dst, dev_out = (buf.ctypes.data, 0) if out is None else (int(buf.data_ptr()), 1)
        return lib().jds_rgb_batch_to_jpeg(c.handle, C.c_void_p(base), on_dev, items_in, n, int(bool(optimize)),
                                           C.c_void_p(dst), cap, dev_out, items, C.byref(need))

    def attempt(c):
        nonlocal cap
        buf = alloc(cap)
        rc = run(c, buf, cap)
        if rc == _abi.JDS_EINVAL and own and need.value > cap:
            cap = int(need.value)
            buf = alloc(cap)
            rc = run(c, buf, cap)
        check(rc)
        return buf

    if ctx is not None:
        buf = attempt(ctx)
    else:
        with lease(device) as c:
            buf = attempt(c)
    info = [_transcode_item_dict(items[i]) for i in range(n)]
    first = _batch_first_error(info)
    if first and errors == 'raise':
        raise ValueError(first)
    outs = []
    for it in info:
        if it['rc'] != 0:
            outs.append(None)
            continue
        v = buf[it['out_off']:it['out_off'] + it['out_len']]
        outs.append(v.tobytes() if out is None else v)
    return outs if errors == 'raise' else (outs, info)


# ------------------------------------------------------------ Pillow resizing --
# (DESIGN.md "Pillow resizing"; Image.thumbnail and reducing_gap go through Pillow's separate
# reduce and are not provided, nor is NEAREST)

def resize_info() -> Tuple[int, int, int]:
    """jds_resize_info: (tile_h, tile_w, max_taps) -- k_resize's default output tile and the taps
    per output sample an axis may need."""
    th, tw, mt = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(lib().jds_resize_info(C.byref(th), C.byref(tw), C.byref(mt)))
    return int(th.value), int(tw.value), int(mt.value)


def _size_arg(size) -> Tuple[int, int]:
    try:
        w, h = size
        w, h = int(w), int(h)
    except (TypeError, ValueError):
        raise ValueError(f'size must be (width, height), got {size!r}') from None
    return w, h


def _box_arg(box):
    """None, or the four C floats of (x0, y0, x1, y1)."""
    if box is None:
        return None
    b = [float(v) for v in box]
    if len(b) != 4:
        raise ValueError(f'box must be (x0, y0, x1, y1), got {box!r}')
    return (C.c_float * 4)(*b)


def _rgb3_arg(image, device: int = 0):
    keep, p, on_dev, H, W, gray = _image_arg(image, device)
    if gray:
        raise ValueError(f'an image is HxWx3, got shape ({H}, {W})')
    return keep, p, on_dev, H, W


def host_rgb_resize(image, size, resample, box=None, with_worst: bool = False):
    """Test aid (jds_selftest_resize): k_resize's tile core in a host tile loop, with the tiles
    the device would use.  with_worst: (image, the largest 255 * sum|k| + 2^21 of the tables
    built -- what a 32-bit accumulator has to hold).  No GPU."""
    keep, p, on_dev, H, W = _rgb3_arg(image)
    if on_dev:
        raise ValueError('host_rgb_resize takes a host array')
    w, h = _size_arg(size)
    out = np.empty((max(h, 0), max(w, 0), 3), np.uint8)
    worst = C.c_int64(0)
    check(lib().jds_selftest_resize(C.c_void_p(p), H, W, _box_arg(box), h, w, _abi.resample_code(resample),
                                    out.ctypes.data if out.size else C.c_void_p(keep.ctypes.data), C.byref(worst)))
    return (out, int(worst.value)) if with_worst else out


def host_resize_coeffs(in_size: int, in0: float, in1: float, out_size: int, resample):
    """Test aid (jds_selftest_resize_coeffs): one axis' table as (ksize, bounds (out_size, 2),
    taps (out_size, ksize))."""
    code = _abi.resample_code(resample)
    ks = C.c_int32(0)
    bounds = np.zeros((int(out_size), 2), np.int32)
    taps = np.zeros(1, np.int32)
    rc = lib().jds_selftest_resize_coeffs(int(in_size), in0, in1, int(out_size), code, C.byref(ks),
                                          bounds.ctypes.data, taps.ctypes.data, 0)
    if rc == _abi.JDS_EINVAL and ks.value > 0:
        taps = np.zeros((int(out_size), int(ks.value)), np.int32)
        rc = lib().jds_selftest_resize_coeffs(int(in_size), in0, in1, int(out_size), code, C.byref(ks),
                                              bounds.ctypes.data, taps.ctypes.data, taps.size)
    check(rc)
    return int(ks.value), bounds, taps


def _tensor_out(out, shape, device: int):
    """A caller's contiguous uint8 device tensor of `shape`, checked."""
    if not _is_tensor(out) or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.element_size() != 1 \
            or not out.is_cuda or out.device.index != int(device):
        raise ValueError(f'out must be a contiguous uint8 {tuple(shape)} tensor on device {int(device)}')
    return out


def rgb_resize(image, size, resample='bilinear', box=None, device: int = 0, out=None):
    """jds_rgb_resize: an HxWx3 uint8 image -- a NumPy array or a contiguous torch tensor on
    `device` -- -> PIL's Image.resize(size, resample, box) of it, byte for byte (k_resize; DESIGN.md
    "Pillow resizing").  size: (width, height), as in Pillow; resample: 'lanczos', 'bilinear',
    'bicubic', 'box', 'hamming' or Pillow's number; box: (x0, y0, x1, y1) in source pixels.  Returns
    an (height, width, 3) array for an array and a device tensor for a tensor; out: a device tensor
    of that shape to write instead.  ValueError for an unknown filter, a size below 1, a box that is
    empty or not within the image, or a reduction beyond the tap cap (resize_info)."""
    keep, p, on_dev, H, W = _rgb3_arg(image, device)
    w, h = _size_arg(size)
    code = _abi.resample_code(resample)
    bx = _box_arg(box)
    if out is not None:
        res = _tensor_out(out, (h, w, 3), device)
        dst, out_dev = int(res.data_ptr()), 1
    elif on_dev:
        import torch
        res = torch.empty((max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=f'cuda:{device}')
        dst, out_dev = int(res.data_ptr()), 1
    else:
        res = np.empty((max(h, 0), max(w, 0), 3), np.uint8)
        dst, out_dev = res.ctypes.data, 0
    if on_dev or out_dev:
        _torch_settled(device)
    with lease(device) as ctx:
        check(lib().jds_rgb_resize(ctx.handle, C.c_void_p(p), on_dev, H, W, bx, h, w, code, C.c_void_p(dst or p),
                                   out_dev))
    return res


def _boxes_arg(boxes, n: int):
    """(per-image boxes or Nones, has-any)."""
    if boxes is None:
        return [None] * n
    boxes = list(boxes)
    if len(boxes) == 4 and all(isinstance(v, (int, float, np.integer, np.floating)) for v in boxes):
        boxes = [tuple(boxes)] * n                   # one box for every image
    if len(boxes) != n:
        raise ValueError(f'{len(boxes)} boxes for {n} images')
    return boxes


def rgb_batch_resize(images, size, resample='bilinear', boxes=None, out=None, device: int = 0, ctx=None):
    """jds_rgb_batch_resize: N device images of any sizes -> one (N, height, width, 3) uint8 device
    tensor, slot i rgb_resize(images[i], ...)'s bytes, by one launch of k_resize_batch on torch's
    current stream (and one before it for images more than 100 times as tall as wide); the call
    returns when they have run.  images: a
    sequence of contiguous HxWx3 uint8 device tensors (views into one allocation -- e.g.
    jpeg_batch_to_rgb(out='device')'s -- are passed by offset, anything else is gathered into one
    buffer first) or an NxHxWx3 device tensor.  boxes: None, one box, or one (or None) per image.
    out: a device tensor of the result's shape.  ctx: a caller-owned Context."""
    import torch
    if _is_tensor(images):
        if images.dim() != 4:
            raise ValueError(f'a batch tensor is NxHxWx3, got shape {tuple(images.shape)}')
        if not images.is_contiguous():
            raise ValueError('a device image must be a contiguous tensor')
        images = [images[i] for i in range(int(images.shape[0]))]
    args = [_rgb3_arg(im, device) for im in images]
    n = len(args)
    if not all(a[2] for a in args):
        raise ValueError('rgb_batch_resize takes device tensors (rgb_resize takes an array)')
    w, h = _size_arg(size)
    code = _abi.resample_code(resample)
    bxs = _boxes_arg(boxes, n)
    base, offs, keep = 0, [], None
    if n:
        bases = {int(a[0].untyped_storage().data_ptr()) for a in args}
        if len(bases) == 1:
            base, keep = bases.pop(), [a[0] for a in args]
            offs = [a[1] - base for a in args]
        else:
            sizes = [a[3] * a[4] * 3 for a in args]
            keep = torch.cat([a[0].reshape(-1) for a in args])
            base, offs = int(keep.data_ptr()), [0] + [int(v) for v in np.cumsum(sizes[:-1])]
    items = (_abi.ResizeItem * max(n, 1))()
    for i, (a, o, b) in enumerate(zip(args, offs, bxs)):
        items[i].rgb_off, items[i].H, items[i].W = int(o), a[3], a[4]
        if b is not None:
            items[i].has_box = 1
            items[i].box = _box_arg(b)
    if out is not None:
        res = _tensor_out(out, (n, h, w, 3), device)
    else:
        res = torch.empty((n, max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=f'cuda:{device}')
    stream = int(torch.cuda.current_stream(device).cuda_stream)

    def run(c):
        return lib().jds_rgb_batch_resize(c.handle, C.c_void_p(base or 1), items, n, h, w, code,
                                          C.c_void_p(int(res.data_ptr()) or 1), C.c_void_p(stream))
    if ctx is not None:
        check(run(ctx))
    else:
        with lease(device) as c:
            check(run(c))
    return res


def jpeg_batch_to_tensor(files, size, resample='bilinear', scale_denom='draft', boxes=None, out='device',
                         errors: str = 'raise', with_info: bool = False, device: int = 0, ctx=None):
    """jds_jpeg_batch_to_tensor: N baseline JPEGs of any sizes -> one (N, height, width, 3) uint8
    tensor: jpeg_batch_to_rgb(render='libjpeg', scale_denom=...)'s decode into scratch of the context,
    then k_resize_batch behind it on the same stream.  With scale_denom='draft' slot i is, byte for
    byte, Pillow's  im = Image.open(f); im.draft('RGB', size); im.convert('RGB').resize(size, resample)
    (draft_denom per file); scale_denom may also be 1, 2, 4, 8 or one per file.  boxes: as
    rgb_batch_resize's, in the coordinates of the image as decoded at its denominator.  A grayscale
    file yields (Y, Y, Y).  out='device': a torch tensor on `device`; None: a NumPy array; or a
    caller's device tensor of the result's shape.  A file that does not parse or whose scan data
    are defective keeps its slot, filled with zeros: errors='raise' raises ValueError naming the
    first such index after the batch has run, errors='return' returns (tensor, bad indices).
    with_info: a dict {'items': per-file dicts with 'scale_denom', 'out_H', 'out_W' of the decode,
    'rounds'} comes last."""
    if errors not in ('raise', 'return'):
        raise ValueError("errors must be 'raise' or 'return'")
    w, h = _size_arg(size)
    code = _abi.resample_code(resample)
    keep, ptrs, lens = _batch_args(files)
    n = len(keep)
    if isinstance(scale_denom, str):
        if scale_denom != 'draft':
            raise ValueError(f"scale_denom {scale_denom!r} is not 'draft', 1, 2, 4 or 8")
        dens_c = None
    else:
        dens, _ = _batch_denoms(scale_denom, n, 'libjpeg')
        dens_c = (C.c_int32 * max(n, 1))(*dens)
    bxs = _boxes_arg(boxes, n)
    boxes_c = None
    if any(b is not None for b in bxs):
        if any(b is None for b in bxs):
            raise ValueError('boxes: one for every file, or none')
        boxes_c = (C.c_float * (4 * n))(*[v for b in bxs for v in _box_arg(b)])
    shape = (n, max(h, 0), max(w, 0), 3)
    if out is None:
        res = np.empty(shape, np.uint8)
        dst, on_dev = res.ctypes.data, 0
    else:
        if isinstance(out, str):
            if out != 'device':
                raise ValueError("out must be None, 'device' or a device tensor of the result's shape")
            import torch
            res = torch.empty(shape, dtype=torch.uint8, device=f'cuda:{device}')
        else:
            res = _tensor_out(out, (n, h, w, 3), device)
        dst, on_dev = int(res.data_ptr()), 1
        _torch_settled(device)
    items = (_abi.JpegBatchItem * max(n, 1))()
    scaled = (_abi.JpegScaledItem * max(n, 1))()
    rounds = C.c_uint32(0)

    def run(c):
        return lib().jds_jpeg_batch_to_tensor(c.handle, ptrs, lens, n, h, w, code, dens_c, boxes_c, C.c_void_p(dst or 1),
                                              n * max(h, 0) * max(w, 0) * 3, on_dev, items, scaled, C.byref(rounds))
    if ctx is not None:
        check(run(ctx))
    else:
        with lease(device) as c:
            check(run(c))
    info = [_batch_item_dict(items[i], max(int(scaled[i].scale_denom), 1)) for i in range(n)]
    first = _batch_first_error(info)
    if first and errors == 'raise':
        raise ValueError(first)
    ret = (res,)
    if errors == 'return':
        ret += ([i for i, it in enumerate(info) if it['rc'] != 0 or it['status'] != 0],)
    if with_info:
        ret += ({'items': info, 'rounds': int(rounds.value)},)
    return ret[0] if len(ret) == 1 else ret


def psnr_ssim_raw(a: np.ndarray, b: np.ndarray, device: int = 0) -> np.ndarray:
    """jds_psnr_ssim: [ssim_R, ssim_G, ssim_B, ssim_Y, mse_Y, mse_RGB] for two HxWx3 uint8 images."""
    a = _u8_image(a)
    b = _u8_image(b)
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    out = np.empty(6, np.float64)
    with lease(device) as ctx:
        check(lib().jds_psnr_ssim(ctx.handle, a.ctypes.data, b.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data))
    return out


def _after(after):
    """`after` of the *_dev calls: None = the caller has synchronised (JDS_AFTER_NONE);
    otherwise a hipStream_t handle, passed unchanged (0 = the HIP null stream, waited for)."""
    return _abi.AFTER_NONE if after is None else C.c_void_p(int(after))


def psnr_ssim_dev(a_ptr: int, b_ptr: int, H: int, W: int, device: int = 0, after=-1) -> np.ndarray:
    """jds_psnr_ssim_dev: psnr_ssim_raw's six values for two HxWx3 uint8 images
    already in device memory (raw device pointers, e.g. torch tensors' data_ptr()).
    after: -1 = wait for the whole device (jds_psnr_ssim_dev); None = the caller
    has synchronised the images; a stream handle = wait only for that stream's
    queued work (jds_psnr_ssim_dev_after)."""
    out = np.empty(6, np.float64)
    with lease(device) as ctx:
        if after == -1:
            check(lib().jds_psnr_ssim_dev(ctx.handle, int(a_ptr), int(b_ptr), int(H), int(W), out.ctypes.data))
        else:
            check(lib().jds_psnr_ssim_dev_after(ctx.handle, int(a_ptr), int(b_ptr), int(H), int(W), out.ctypes.data,
                                                _after(after)))
    return out


def psnr_ssim_batch_dev(a_ptrs, b_ptrs, H: int, W: int, device: int = 0, after=None, ctx=None) -> np.ndarray:
    """jds_psnr_ssim_batch_dev: [n, 6] (psnr_ssim_raw's six values) for n
    device-resident image pairs (a_ptrs[i], b_ptrs[i]) of one size, run together
    on the GPU (the batch sweep's per-item SSIM).  after as in psnr_ssim_dev
    (None: the caller has synchronised).  ctx: a caller-owned Context of that
    device (e.g. with its own SSIM scratch budget) instead of a pooled one."""
    n = len(a_ptrs)
    if len(b_ptrs) != n:
        raise ValueError('a_ptrs and b_ptrs differ in length')
    out = np.empty((n, 6), np.float64)
    if n == 0:
        return out
    pa = (C.c_void_p * n)(*[int(p) for p in a_ptrs])
    pb = (C.c_void_p * n)(*[int(p) for p in b_ptrs])
    if ctx is not None:
        check(lib().jds_psnr_ssim_batch_dev(ctx.handle, n, pa, pb, int(H), int(W), out.ctypes.data, _after(after)))
        return out
    with lease(device) as c:
        check(lib().jds_psnr_ssim_batch_dev(c.handle, n, pa, pb, int(H), int(W), out.ctypes.data, _after(after)))
    return out


def magnitude_bits_f32_dev(coeffs_ptr: int, n_coeffs: int, device: int = 0, after=None) -> float:
    """jds_magnitude_bits_f32_dev: NumPy's float32 np.sum of magnitude_bits
    (utils/metrics.py:77-78) over n_coeffs device-resident int16 coefficients.
    after as in psnr_ssim_dev: None = the caller has synchronised the coefficients;
    a stream handle = wait for that stream's queued work."""
    out = C.c_double()
    with lease(device) as ctx:
        check(lib().jds_magnitude_bits_f32_dev(ctx.handle, int(coeffs_ptr), int(n_coeffs), C.byref(out),
                                               _after(after)))
    return float(out.value)


def magnitude_bits_f32_batch_dev(coeffs_ptr: int, n_items: int, n_coeffs: int, item_stride: int,
                                 device: int = 0, after=None) -> np.ndarray:
    """jds_magnitude_bits_f32_batch_dev: magnitude_bits_f32_dev for n_items
    coefficient arrays at coeffs_ptr + 2 * i * item_stride bytes, one host wait
    (after as magnitude_bits_f32_dev's)."""
    out = np.empty(n_items, np.float64)
    if n_items == 0:
        return out
    with lease(device) as ctx:
        check(lib().jds_magnitude_bits_f32_batch_dev(ctx.handle, int(coeffs_ptr), int(n_items), int(n_coeffs),
                                                     int(item_stride), out.ctypes.data, _after(after)))
    return out


# ----------------------------------------------------------- per-stage ops

def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def stage_rgb_ycbcr(x: np.ndarray, inverse: bool) -> np.ndarray:
    x = _f64(x)
    if x.shape[-1] != 3:
        raise IndexError('index 2 is out of bounds for axis 2')
    out = np.empty_like(x)
    fn = lib().jds_stage_ycbcr_to_rgb if inverse else lib().jds_stage_rgb_to_ycbcr
    with lease() as ctx:
        check(fn(ctx.handle, x.ctypes.data, out.ctypes.data, x.size // 3))
    return out


def stage_subsample(cb: np.ndarray, cr: np.ndarray, mode: str, prefilter: bool, gauss=None):
    cb, cr = _f64(cb), _f64(cr)
    H, W = cb.shape
    oh = H // 2 if mode == '4:2:0' else H
    ocb = np.empty((oh, W // 2), np.float64)
    ocr = np.empty((oh, W // 2), np.float64)
    g = _taps(gauss)
    with lease() as ctx:
        check(lib().jds_stage_subsample(ctx.handle, cb.ctypes.data, cr.ctypes.data, H, W,
                                        _abi.MODE_CODES[mode], 1 if prefilter else 0, g.ctypes.data,
                                        ocb.ctypes.data, ocr.ctypes.data))
    return ocb, ocr


def stage_resize(x: np.ndarray, H: int, W: int, nearest: bool) -> np.ndarray:
    x = _f64(x)
    out = np.empty((H, W), np.float64)
    with lease() as ctx:
        check(lib().jds_stage_upsample(ctx.handle, x.ctypes.data, x.shape[0], x.shape[1], H, W,
                                       1 if nearest else 0, out.ctypes.data))
    return out


def stage_block(x: np.ndarray, op: int) -> np.ndarray:
    """op: 0 dct2, 1 idct2, 2 encode_block, 3 decode_block on (..., 8, 8) or (..., 16, 16)."""
    x = _f64(x)
    if x.ndim < 2 or x.shape[-2:] not in ((8, 8), (16, 16)):
        raise ValueError(f'the MI355X block transforms are 8x8 and 16x16 (got {x.shape})')
    b = x.shape[-1]
    out = np.empty_like(x)
    with lease() as ctx:
        check(lib().jds_stage_block_dct_n(ctx.handle, x.ctypes.data, out.ctypes.data, x.size // (b * b), b, op))
    return out


def stage_quant(x: np.ndarray, q: np.ndarray, dequant: bool) -> np.ndarray:
    q = _f64(q)
    if q.shape not in ((8, 8), (16, 16)) or x.shape[-2:] != q.shape:
        # NumPy's broadcast error for c / Q (engines/quantizer.py:24)
        fmt = lambda s: '(' + ','.join(str(d) for d in s) + (',)' if len(s) == 1 else ')')
        raise ValueError(f'operands could not be broadcast together with shapes {fmt(x.shape)} {fmt(q.shape)} ')
    if dequant:
        x = np.ascontiguousarray(x, dtype=np.int16)
        out = np.empty(x.shape, np.float64)
    else:
        x = _f64(x)
        out = np.empty(x.shape, np.int16)
    with lease() as ctx:
        check(lib().jds_stage_quantize_n(ctx.handle, x.ctypes.data, q.ctypes.data, q.size, out.ctypes.data,
                                         x.size, 1 if dequant else 0))
    return out
