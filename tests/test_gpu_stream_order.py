"""GPU checks of stream ordering (INTEGRATION.md "Stream ordering"): every call that reads or writes
a torch tensor, run while torch's current stream still holds work on that tensor.

A context's stream waits for nothing torch has queued, so a call whose source or destination is a
torch tensor has to settle torch's current stream first (codec._torch_settled), take the stream
(`stream=`) or run on torch's stream itself.  Each test here queues work that outlasts the call by
a wide margin (Busy), queues a fill or a copy of the tensor behind it, and calls at once:

  output side     out.fill_(0x5A) is pending on the caller's tensor: the result is the idle-device
                  result, and nothing outside the images changes
  recycled block  a tensor of the size the call allocates is filled and freed while the fill is
                  pending; out='device' gets that very block back from the caching allocator
  input side      copy_ of new content into the source tensor is pending: the result is the new
                  content's
  launch-only     jpeg_inverse_dev, jpeg_render_dev, rgb_forward_dev on a non-default torch stream
                  that still has to produce the input and pre-fill the output

and one representative of each family again under a non-default current stream.  The pending work
is sized per test from the call's own wall time on an idle device (at least 20 times that and at
least 50 ms, measured again with events around the queued work itself), and an event behind it must
still be pending when the call starts: a test that could not lose the race fails.  Every comparison
is an equality with the same call on an idle device, and one case per family with Pillow's bytes.
Small files only."""
import contextlib
import math
import time

import numpy as np
import pytest

import pjpeg_cases as pc
from test_jpeg_forward_cpu import image, of_mode, pillow_save
from test_jpeg_render_cpu import pillow_file, pillow_pixels
from test_resize_cpu import pillow as pillow_resize, pillow_draft_resize

pytestmark = pytest.mark.gpu

FILL = 0x5A
LEAD = 64                                                    # guard bytes in front of and behind a caller's buffer
STREAMS = ['default', 'side']


@pytest.fixture(scope='module', autouse=True)
def gpu():
    from jds import build, _abi
    build.build()
    assert _abi.device_count() >= 1, 'no HIP device: the MI355X path has no CPU fallback'


class Busy:
    """Work for torch's current stream: in-place passes over a 512 MiB buffer, allocated once.  One
    pass is timed with events here; queue(ms) issues passes worth 1.5 times `ms` by that figure and
    returns a function that gives the time they really took (events around them) once they have run."""

    def __init__(self):
        import torch
        self.buf = torch.zeros(128 << 20, dtype=torch.int32, device='cuda')
        self._passes(4)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._passes(32)
        b.record()
        b.synchronize()
        self.pass_ms = a.elapsed_time(b) / 32
        assert self.pass_ms > 0

    def _passes(self, n):
        for _ in range(n):
            self.buf.add_(1)

    def queue(self, ms):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._passes(math.ceil(1.5 * ms / self.pass_ms))
        b.record()
        return lambda: a.elapsed_time(b)


@pytest.fixture(scope='module')
def busy():
    b = Busy()
    print(f'\nBusy: one pass over {b.buf.numel() * 4 >> 20} MiB takes {b.pass_ms:.3f} ms')
    return b


@contextlib.contextmanager
def on(stream):
    """torch's default stream, or a new non-default one as the current stream."""
    import torch
    if stream == 'default':
        yield
    else:
        with torch.cuda.stream(torch.cuda.Stream()):
            yield


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared images are read-only)


def same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def idle(call, prepare, sync):
    """The call twice on an idle device, each time after `prepare` has run: the first run loads code
    objects and grows the context's buffers, the second -> (its result, its wall time in ms)."""
    for _ in range(2):
        prepare()
        sync()
        t0 = time.perf_counter()
        r = call()
        sync()
        ms = (time.perf_counter() - t0) * 1e3
    return r, ms


class Pending:
    """Busy work of max(20 * idle_ms, 50) ms on the current stream, `then()` queued behind it."""

    def __init__(self, busy, name, idle_ms, then):
        import torch
        self.name, self.idle_ms, self.need = name, idle_ms, max(20.0 * idle_ms, 50.0)
        self.span = busy.queue(self.need)
        then()
        self.ev = torch.cuda.Event()
        self.ev.record()

    def still(self):
        """Immediately before the call under test."""
        assert not self.ev.query(), f'{self.name}: the pending work had ended before the call began'

    def lasted(self):
        """After everything has run: the pending work took what the rule asks for."""
        ms = self.span()
        print(f'\n{self.name}: idle call {self.idle_ms:.3f} ms, pending work {ms:.1f} ms (at least {self.need:.1f})')
        assert ms >= self.need, f'{self.name}: the pending work lasted {ms:.1f} ms, not {self.need:.1f}'


def race(busy, name, call, host, pending, stale=None, sync=None):
    """-> (host(result) of the call on an idle device after pending() has run, host(result) of the
    call made while the busy work and pending() behind it are still queued).  stale() puts the
    tensors into a state neither result contains before the second part."""
    import torch
    sync = sync or torch.cuda.synchronize
    r, idle_ms = idle(call, pending, sync)
    exp = host(r)
    del r
    if stale is not None:
        stale()
    torch.cuda.synchronize()
    p = Pending(busy, name, idle_ms, pending)
    p.still()
    r = call()
    sync()
    got = host(r)
    p.lasted()
    return exp, got


def recycled(busy, name, call, first_view, host):
    """The recycled block: -> (host(result) on an idle device, host(result) of the call that got
    the block of a tensor freed with a fill still pending on it)."""
    import torch
    r, idle_ms = idle(call, lambda: None, torch.cuda.synchronize)
    exp = host(r)
    nbytes = first_view(r).untyped_storage().nbytes()        # what the call allocates
    del r
    t = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    ptr = t.data_ptr()
    p = Pending(busy, name, idle_ms, lambda: t.fill_(FILL))
    del t
    p.still()
    r = call()
    v = first_view(r)
    assert v.untyped_storage().data_ptr() == ptr and v.data_ptr() == ptr, f'{name}: the allocator did not recycle the block'
    torch.cuda.synchronize()
    got = host(r)
    p.lasted()
    return exp, got, nbytes


def guarded(nbytes):
    import torch
    return torch.empty(LEAD + nbytes + LEAD, dtype=torch.uint8, device='cuda')


def untouched(host, spans):
    """Every byte of `host` outside the (offset, length) spans is still FILL."""
    keep = np.ones(host.size, bool)
    for o, n in spans:
        keep[o:o + n] = False
    return bool(np.all(host[keep] == FILL))


def baseline_files():
    return [pillow_file(31, 45, '4:2:0'), pillow_file(9, 9, '4:4:4'), pillow_file(37, 53, 'L'), pillow_file(33, 35, '4:2:2')]


def progressive_files():
    return [pc.pillow_pair(h, w, ss, r, 75)[1] for h, w, ss, r in ((17, 33, 0, 0), (37, 53, 1, 0), (40, 56, 2, 0), (24, 40, 'L', 0))]


TWINS = [(37, 45, 'noise', '4:2:0', 75), (17, 33, 'ramp', '4:4:4', 90), (48, 64, 'two-level', '4:2:2', 50)]


def twin_files(optimize):
    """Pillow's files of three images, plain or with optimised tables: each kind transcodes to the other."""
    return [pillow_save(image(h, w, kind), mode, q, optimize) for h, w, kind, mode, q in TWINS]


def forward_images(seed=0):
    return [image(37, 45, 'noise', seed), image(17, 33, 'ramp', seed), of_mode(image(48, 64, 'noise', seed), 'gray'),
            image(9, 17, 'two-level', seed)]


FWD_Q, FWD_SS = [75, 90, 60, 30], ['4:2:0', '4:4:4', '4:2:0', '4:2:2']


# ---------------------------------------------------------------- 1. output side --

def single_to_out(busy, name, stream, fn, data, h, w, **kw):
    """jpeg_to_rgb / pjpeg_to_rgb into a view between guard bytes -> the image."""
    n = h * w * 3
    with on(stream):
        buf = guarded(n)
        out = buf[LEAD:LEAD + n].view(h, w, 3)
        exp, got = race(busy, name, lambda: fn(data, out=out, **kw), lambda r: buf.cpu().numpy(),
                        lambda: buf.fill_(FILL), lambda: buf.zero_())
    assert np.array_equal(got, exp), name
    assert untouched(got, [(LEAD, n)]), name
    return got[LEAD:LEAD + n].reshape(h, w, 3)


@pytest.mark.parametrize('stream,render,denom', [('default', 'reference', 1), ('default', 'libjpeg', 1),
                                                  ('default', 'libjpeg', 2), ('side', 'libjpeg', 1)])
def test_jpeg_to_rgb_out_tensor_with_a_fill_pending(busy, stream, render, denom):
    from jds import codec
    data = pillow_file(31, 45, '4:2:0')
    h, w = codec.jpeg_scaled_size(31, 45, denom)
    img = single_to_out(busy, f'jpeg_to_rgb[{stream}-{render}-{denom}]', stream, codec.jpeg_to_rgb, data, h, w,
                        render=render, scale_denom=denom)
    assert np.array_equal(img, codec.jpeg_to_rgb(data, render=render, scale_denom=denom))
    if render == 'libjpeg' and denom == 1:
        assert np.array_equal(img, pillow_pixels(data))


@pytest.mark.parametrize('stream,denom', [('default', 1), ('default', 4), ('side', 1)])
def test_pjpeg_to_rgb_out_tensor_with_a_fill_pending(busy, stream, denom):
    from jds import codec
    data = pc.pillow_pair(37, 53, 1, 0, 75)[1]
    h, w = codec.jpeg_scaled_size(37, 53, denom)
    img = single_to_out(busy, f'pjpeg_to_rgb[{stream}-{denom}]', stream, codec.pjpeg_to_rgb, data, h, w, scale_denom=denom)
    assert np.array_equal(img, codec.pjpeg_to_rgb(data, scale_denom=denom))
    if denom == 1:
        assert np.array_equal(img, pc.pillow_rgb(data))


def batch_rgb_to_out(busy, name, stream, fn, files, pillow, **kw):
    import torch
    alone, info = fn(files, out=None, with_info=True, **kw)
    spans = [(LEAD * 4 + it['rgb_off'], it['out_H'] * it['out_W'] * 3) for it in info['items']]
    with on(stream):
        buf = torch.empty(LEAD * 4 + info['rgb_bytes'] + LEAD, dtype=torch.uint8, device='cuda')
        out = buf[LEAD * 4:LEAD * 4 + info['rgb_bytes']]     # (at a multiple of 256, as the images are)
        exp, got = race(busy, name, lambda: fn(files, out=out, **kw), lambda r: (buf.cpu().numpy(), [v.cpu().numpy() for v in r]),
                        lambda: buf.fill_(FILL), lambda: buf.zero_())
    assert same(got, exp), name
    assert untouched(got[0], spans), name
    for i, (o, n) in enumerate(spans):
        assert np.array_equal(got[0][o:o + n], alone[i].reshape(-1)) and np.array_equal(got[1][i], alone[i]), (name, i)
        if pillow:
            assert np.array_equal(got[1][i], pillow_pixels(files[i])), (name, i)


@pytest.mark.parametrize('stream,kw', [('default', dict(render='libjpeg', scale_denom=[1, 2, 1, 4])),
                                       ('default', dict()), ('side', dict(render='libjpeg'))])
def test_jpeg_batch_to_rgb_out_tensor_with_a_fill_pending(busy, stream, kw):
    from jds import codec
    batch_rgb_to_out(busy, f'jpeg_batch_to_rgb[{stream}-{len(kw)}]', stream, codec.jpeg_batch_to_rgb, baseline_files(),
                     kw == dict(render='libjpeg'), **kw)


@pytest.mark.parametrize('stream', STREAMS)
def test_pjpeg_batch_to_rgb_out_tensor_with_a_fill_pending(busy, stream):
    from jds import codec
    batch_rgb_to_out(busy, f'pjpeg_batch_to_rgb[{stream}]', stream, codec.pjpeg_batch_to_rgb, progressive_files(), True)


def files_to_out(busy, name, stream, call, alone, items):
    """A transcode-shaped call (files into a caller's 1-D tensor, errors='items') -> the files."""
    import torch
    need = max(-(-(it['out_off'] + it['out_len']) // 256) * 256 for it in items)
    spans = [(LEAD * 4 + it['out_off'], it['out_len']) for it in items]
    with on(stream):
        buf = torch.empty(LEAD * 4 + need + LEAD, dtype=torch.uint8, device='cuda')
        out = buf[LEAD * 4:LEAD * 4 + need]
        exp, got = race(busy, name, lambda: call(out), lambda r: (buf.cpu().numpy(), [v.cpu().numpy().tobytes() for v in r[0]], r[1]),
                        lambda: buf.fill_(FILL), lambda: buf.zero_())
    assert same(got, exp), name
    assert got[2] == items and got[1] == alone, name
    assert untouched(got[0], spans), name
    for (o, n), f in zip(spans, alone):
        assert got[0][o:o + n].tobytes() == f, name
    return got[1]


@pytest.mark.parametrize('stream', STREAMS)
def test_jpeg_batch_transcode_out_tensor_with_a_fill_pending(busy, stream):
    from jds import codec
    files = twin_files(False)
    alone, items = codec.jpeg_batch_transcode(files, optimize=True, errors='items')
    got = files_to_out(busy, f'jpeg_batch_transcode[{stream}]', stream,
                       lambda out: codec.jpeg_batch_transcode(files, optimize=True, out=out, errors='items'), alone, items)
    assert got == twin_files(True)                           # Pillow's own files of the other kind


def test_jpeg_batch_transform_out_tensor_with_a_fill_pending(busy):
    from jds import codec
    files, ops = twin_files(False), ['none', 'rot180', 'hflip']
    alone, items = codec.jpeg_batch_transform(files, ops, trim=True, errors='items')
    got = files_to_out(busy, 'jpeg_batch_transform', 'default',
                       lambda out: codec.jpeg_batch_transform(files, ops, trim=True, out=out, errors='items'), alone, items)
    assert got[0] == twin_files(True)[0]                     # 'none' is the transcode: Pillow's optimised file
    assert got[1] == codec.jpeg_transform(files[1], 'rot180', trim=True)


def test_pjpeg_batch_transcode_out_tensor_with_a_fill_pending(busy):
    from jds import codec
    files = progressive_files()
    alone, items = codec.pjpeg_batch_transcode(files, optimize=False, errors='items')
    got = files_to_out(busy, 'pjpeg_batch_transcode', 'default',
                       lambda out: codec.pjpeg_batch_transcode(files, optimize=False, out=out, errors='items'), alone, items)
    arr, _, base, kw = pc.pillow_pair(17, 33, 0, 0, 75)
    assert got[0] == base == pc.save(arr, **dict(kw))        # Pillow's baseline file of the same array


@pytest.mark.parametrize('stream', STREAMS)
def test_rgb_batch_to_jpeg_host_inputs_out_tensor_with_a_fill_pending(busy, stream):
    from jds import codec
    imgs = forward_images()
    alone, items = codec.rgb_batch_to_jpeg(imgs, FWD_Q, FWD_SS, optimize=True, errors='items')
    got = files_to_out(busy, f'rgb_batch_to_jpeg[host-{stream}]', stream,
                       lambda out: codec.rgb_batch_to_jpeg(imgs, FWD_Q, FWD_SS, optimize=True, out=out, errors='items'),
                       alone, items)
    assert got[0] == pillow_save(imgs[0], FWD_SS[0], FWD_Q[0], True)
    assert got[2] == pillow_save(imgs[2], 'gray', FWD_Q[2], True)


# -------------------------------------------------------------- 2. recycled block --

def views_host(r):
    return [v.cpu().numpy() for v in r]


@pytest.mark.parametrize('stream', STREAMS)
def test_jpeg_batch_to_rgb_device_in_a_recycled_block(busy, stream):
    from jds import codec
    files = baseline_files()
    with on(stream):
        exp, got, nbytes = recycled(busy, f'jpeg_batch_to_rgb[device-{stream}]',
                                    lambda: codec.jpeg_batch_to_rgb(files, out='device', render='libjpeg'), lambda r: r[0], views_host)
    assert nbytes == codec.jpeg_batch_layout(files)[1]
    assert same(got, exp)
    for f, im in zip(files, got):
        assert np.array_equal(im, pillow_pixels(f))


def test_pjpeg_batch_to_rgb_device_in_a_recycled_block(busy):
    from jds import codec
    files = progressive_files()
    exp, got, nbytes = recycled(busy, 'pjpeg_batch_to_rgb[device]', lambda: codec.pjpeg_batch_to_rgb(files, out='device'),
                                lambda r: r[0], views_host)
    assert nbytes == codec.pjpeg_batch_to_rgb(files, out=None, with_info=True)[1]['rgb_bytes']
    assert same(got, exp)
    for f, im in zip(files, got):
        assert np.array_equal(im, pc.pillow_rgb(f))


def files_host(r):
    return [v.cpu().numpy().tobytes() for v in r[0]], r[1]


def reported_need(items):
    return max(-(-(it['out_off'] + it['out_len']) // 256) * 256 for it in items)


@pytest.mark.parametrize('stream', STREAMS)
def test_jpeg_batch_transcode_device_in_a_recycled_block(busy, stream):
    """The block is of the size the call allocates (its first guess, which is at least the need it reports)."""
    from jds import codec
    files = twin_files(False)
    with on(stream):
        exp, got, nbytes = recycled(busy, f'jpeg_batch_transcode[device-{stream}]',
                                    lambda: codec.jpeg_batch_transcode(files, optimize=True, out='device', errors='items'),
                                    lambda r: r[0][0], files_host)
    assert nbytes >= reported_need(got[1])
    assert same(got, exp) and got[0] == twin_files(True)


def test_jpeg_batch_transform_device_in_a_recycled_block(busy):
    from jds import codec
    files, ops = twin_files(False), ['rot180', 'none', 'vflip']
    exp, got, nbytes = recycled(busy, 'jpeg_batch_transform[device]',
                                lambda: codec.jpeg_batch_transform(files, ops, trim=True, out='device', errors='items'),
                                lambda r: r[0][0], files_host)
    assert nbytes >= reported_need(got[1])
    assert same(got, exp) and got[0] == codec.jpeg_batch_transform(files, ops, trim=True) and got[0][1] == twin_files(True)[1]


def test_pjpeg_batch_transcode_device_in_a_recycled_block(busy):
    from jds import codec
    files = progressive_files()
    exp, got, nbytes = recycled(busy, 'pjpeg_batch_transcode[device]',
                                lambda: codec.pjpeg_batch_transcode(files, optimize=False, out='device', errors='items'),
                                lambda r: r[0][0], files_host)
    assert nbytes >= reported_need(got[1])
    assert same(got, exp) and got[0][0] == pc.pillow_pair(17, 33, 0, 0, 75)[2]


@pytest.mark.parametrize('stream', STREAMS)
def test_rgb_batch_to_jpeg_host_inputs_device_in_a_recycled_block(busy, stream):
    from jds import codec
    imgs = forward_images()
    with on(stream):
        exp, got, nbytes = recycled(busy, f'rgb_batch_to_jpeg[host-device-{stream}]',
                                    lambda: codec.rgb_batch_to_jpeg(imgs, FWD_Q, FWD_SS, out='device', errors='items'),
                                    lambda r: r[0][0], files_host)
    assert nbytes >= reported_need(got[1])
    assert same(got, exp)
    assert got[0] == [pillow_save(im, ss, q) for im, ss, q in zip(imgs, ['4:2:0', '4:4:4', 'gray', '4:2:2'], FWD_Q)]


# ----------------------------------------------------------------- 3. input side --

@pytest.mark.parametrize('stream', STREAMS)
def test_rgb_to_jpeg_with_a_copy_into_the_image_pending(busy, stream):
    import torch
    from jds import codec
    old, new = image(37, 45, 'noise', 1), image(37, 45, 'noise', 2)
    with on(stream):
        d_old, d_new = to_dev(old), to_dev(new)
        t = torch.empty_like(d_new)
        exp, got = race(busy, f'rgb_to_jpeg[{stream}]', lambda: codec.rgb_to_jpeg(t, 75, '4:2:0'), lambda r: r,
                        lambda: t.copy_(d_new), lambda: t.copy_(d_old))
    assert got == exp == pillow_save(new, '4:2:0', 75)


@pytest.mark.parametrize('stream,layout', [('default', 'views'), ('default', 'separate'), ('side', 'separate')])
def test_rgb_batch_to_jpeg_device_inputs_with_copies_pending(busy, stream, layout):
    import torch
    from jds import codec
    old, new = forward_images(1), forward_images(2)
    with on(stream):
        if layout == 'views':
            offs = np.cumsum([0] + [a.size for a in new])
            d_old, d_new = (to_dev(np.concatenate([a.reshape(-1) for a in v])) for v in (old, new))
            pool = torch.empty_like(d_new)
            ts = [pool[offs[i]:offs[i + 1]].view(a.shape) for i, a in enumerate(new)]
            pending, stale = (lambda: pool.copy_(d_new)), (lambda: pool.copy_(d_old))
        else:
            d_old, d_new = [to_dev(a) for a in old], [to_dev(a) for a in new]
            ts = [torch.empty_like(a) for a in d_new]
            pending = lambda: [t.copy_(a) for t, a in zip(ts, d_new)]

            def stale():                                     # also the block the call gathers into, if it is recycled
                torch.zeros(sum(t.numel() for t in ts), dtype=torch.uint8, device='cuda')
                for t, a in zip(ts, d_old):
                    t.copy_(a)
        exp, got = race(busy, f'rgb_batch_to_jpeg[{layout}-{stream}]', lambda: codec.rgb_batch_to_jpeg(ts, FWD_Q, FWD_SS),
                        lambda r: r, pending, stale)
    assert got == exp == codec.rgb_batch_to_jpeg(new, FWD_Q, FWD_SS)
    assert got[0] == pillow_save(new[0], FWD_SS[0], FWD_Q[0])


@pytest.mark.parametrize('stream', STREAMS)
def test_rgb_resize_with_a_copy_into_the_image_pending(busy, stream):
    import torch
    from PIL import Image
    from jds import codec
    old, new, size = image(37, 45, 'noise', 1), image(37, 45, 'noise', 2), (23, 19)
    with on(stream):
        d_old, d_new = to_dev(old), to_dev(new)
        t = torch.empty_like(d_new)
        exp, got = race(busy, f'rgb_resize[{stream}]', lambda: codec.rgb_resize(t, size, 'bicubic'), lambda r: r.cpu().numpy(),
                        lambda: t.copy_(d_new), lambda: t.copy_(d_old))
    assert np.array_equal(got, exp) and np.array_equal(got, pillow_resize(new, size, Image.BICUBIC))


def test_rgb_resize_of_an_array_into_a_tensor_with_a_fill_pending(busy):
    from PIL import Image
    from jds import codec
    img, size = image(37, 45, 'noise', 2), (23, 19)
    n = size[0] * size[1] * 3
    buf = guarded(n)
    out = buf[LEAD:LEAD + n].view(size[1], size[0], 3)
    exp, got = race(busy, 'rgb_resize[array-to-tensor]', lambda: codec.rgb_resize(img, size, 'bicubic', out=out),
                    lambda r: buf.cpu().numpy(), lambda: buf.fill_(FILL), lambda: buf.zero_())
    assert np.array_equal(got, exp) and untouched(got, [(LEAD, n)])
    assert np.array_equal(got[LEAD:LEAD + n].reshape(size[1], size[0], 3), pillow_resize(img, size, Image.BICUBIC))


@pytest.mark.parametrize('stream,layout', [('default', 'views'), ('default', 'separate'), ('side', 'views')])
def test_rgb_batch_resize_with_copies_pending(busy, stream, layout):
    import torch
    from PIL import Image
    from jds import codec
    shapes, size = [(37, 45), (17, 33), (48, 64)], (20, 18)
    old, new = ([image(h, w, 'noise', s) for h, w in shapes] for s in (1, 2))
    with on(stream):
        if layout == 'views':
            offs = np.cumsum([0] + [a.size for a in new])
            d_old, d_new = (to_dev(np.concatenate([a.reshape(-1) for a in v])) for v in (old, new))
            pool = torch.empty_like(d_new)
            ts = [pool[offs[i]:offs[i + 1]].view(a.shape) for i, a in enumerate(new)]
            pending, stale = (lambda: pool.copy_(d_new)), (lambda: pool.copy_(d_old))
        else:
            d_old, d_new = [to_dev(a) for a in old], [to_dev(a) for a in new]
            ts = [torch.empty_like(a) for a in d_new]
            pending = lambda: [t.copy_(a) for t, a in zip(ts, d_new)]
            stale = lambda: [t.copy_(a) for t, a in zip(ts, d_old)]
        exp, got = race(busy, f'rgb_batch_resize[{layout}-{stream}]', lambda: codec.rgb_batch_resize(ts, size, 'lanczos'),
                        lambda r: r.cpu().numpy(), pending, stale)
    assert np.array_equal(got, exp)
    for i, a in enumerate(new):
        assert np.array_equal(got[i], pillow_resize(a, size, Image.LANCZOS)), i


@pytest.mark.parametrize('stream', STREAMS)
def test_jpeg_batch_to_tensor_out_tensor_with_a_fill_pending(busy, stream):
    from PIL import Image
    from jds import codec
    files, size = [pillow_file(65, 257, '4:2:0', 30)] + baseline_files()[:3], (16, 16)
    n = len(files) * size[0] * size[1] * 3
    with on(stream):
        buf = guarded(n)
        out = buf[LEAD:LEAD + n].view(len(files), size[1], size[0], 3)
        exp, got = race(busy, f'jpeg_batch_to_tensor[{stream}]', lambda: codec.jpeg_batch_to_tensor(files, size, 'bilinear', out=out),
                        lambda r: buf.cpu().numpy(), lambda: buf.fill_(FILL), lambda: buf.zero_())
    assert np.array_equal(got, exp) and untouched(got, [(LEAD, n)])
    res = got[LEAD:LEAD + n].reshape(len(files), size[1], size[0], 3)
    assert np.array_equal(res, codec.jpeg_batch_to_tensor(files, size, 'bilinear', out=None))
    for i, f in enumerate(files):
        assert np.array_equal(res[i], pillow_draft_resize(f, size, Image.BILINEAR)), i


def test_jpeg_batch_to_tensor_device_in_a_recycled_block(busy):
    from jds import codec
    files, size = baseline_files(), (16, 16)
    exp, got, nbytes = recycled(busy, 'jpeg_batch_to_tensor[device]', lambda: codec.jpeg_batch_to_tensor(files, size, 'bilinear'),
                                lambda r: r, lambda r: r.cpu().numpy())
    assert nbytes == len(files) * 16 * 16 * 3
    assert np.array_equal(got, exp) and np.array_equal(got, codec.jpeg_batch_to_tensor(files, size, 'bilinear', out=None))


# ------------------------------------------------------------ 4. launch-only calls --

@pytest.mark.parametrize('what', ['inverse', 'render', 'render-half', 'forward'])
def test_launch_only_calls_on_a_stream_that_still_produces_their_input(busy, what):
    """jpeg_inverse_dev, jpeg_render_dev (also scaled) and rgb_forward_dev take `stream=`: a
    non-default torch stream with the busy work, the copy that produces the input and the fill of
    the output queued on it.  After synchronising that stream the output is the host core's."""
    import torch
    from jds import codec, entropy
    if what == 'forward':
        img = image(37, 45, 'noise')
        want, info = codec.host_rgb_forward(img, 75, '4:2:0')
        src, dt, fill = img.reshape(-1), torch.int16, 0x5A5A
        launch = lambda i, o, s: codec.rgb_forward_dev(info, i, o, stream=s)
    else:
        d = entropy.decode_jpeg(pillow_file(31, 45, '4:2:0'))
        args = (d['coeffs'], d['H'], d['W'], d['mode'], d['qtables'], d['grids'])
        src, dt, fill = d['coeffs'], torch.uint8, FILL
        if what == 'inverse':
            want = codec.host_jpeg_inverse(*args)
            launch = lambda i, o, s: codec.jpeg_inverse_dev(d, i, o, stream=s)
        else:
            den = 2 if what == 'render-half' else 1
            want = codec.host_jpeg_render(*args, render='libjpeg', scale_denom=den)
            launch = lambda i, o, s: codec.jpeg_render_dev(d, i, o, render='libjpeg', stream=s, scale_denom=den)
    want = np.asarray(want).reshape(-1)
    d_src = to_dev(src)
    torch.cuda.synchronize()
    guard = 64                                               # entries: int16 planes stay 16-byte aligned
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        inp = torch.zeros_like(d_src)
        out = torch.zeros(guard + want.size + guard, dtype=dt, device='cuda')

        def pending():
            inp.copy_(d_src)
            out.fill_(fill)

        def stale():
            inp.zero_()
            out.zero_()
        exp, got = race(busy, f'{what}_dev', lambda: launch(inp.data_ptr(), out.data_ptr() + guard * out.element_size(), s.cuda_stream),
                        lambda r: out.cpu().numpy(), pending, stale, sync=s.synchronize)
    assert np.array_equal(got, exp)
    assert np.all(got[:guard] == fill) and np.all(got[guard + want.size:] == fill)
    assert np.array_equal(got[guard:guard + want.size], want)
