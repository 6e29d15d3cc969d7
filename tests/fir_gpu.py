"""What the FIR filter's GPU tests share (tests/test_gpu_fir.py, test_gpu_stream_long.py, test_gpu_multi_ctx.py, tests/tools/fuzz_fir.py): the
CPU statement built once per process, a bit view, the block call in every view with guard words around the signals, the streaming handle, and a
restatement of the library's tile rule.  Every comparison made with these is bit equality against tests/fir_ref/ref_fir.c."""
import tempfile

import numpy as np

import fir_ref

PAD = 8        # frames behind every destination signal that must stay untouched
SENTINEL = np.float32(-12345.0)
# (channels, streams, source layout, destination layout, shared source): interleaved and planar views on both sides, stream_stride = 0
CONFIGS = ((1, 1, "i", "i", False), (2, 1, "i", "i", False), (1, 3, "p", "p", False), (2, 3, "p", "p", False),
           (2, 3, "i", "p", False), (2, 1, "p", "i", False), (2, 3, "i", "i", True), (1, 3, "p", "p", True))
WAVES = {512: 8, 1024: 8, 2048: 7, 4096: 3}        # Fir<N>::kWaves, waves (stream-channel x tile items) per workgroup
RESIDENT = {512: 16, 1024: 8, 2048: 7, 4096: 3}    # Fir<N>::kResident, waves a CU holds
MIN_TILE = 8                                       # NAE_FIR_MIN_TILE

_statement = None


def statement():
    """the CPU statement's library, compiled once per process"""
    global _statement
    if _statement is None:
        tmp = tempfile.TemporaryDirectory(prefix="ref_fir_gpu")
        _statement = (fir_ref.build(tmp.name), tmp)
    return _statement[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(rng, n_streams, n, ch, shared=False):
    x = rng.uniform(-1, 1, (n_streams, n, ch)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def pick_tile(n_fft, blocks, n_sc, n_cu=256):
    """nae_pick_fir_tile restated: (blocks per tile, tiles per stream-channel) of a launch with fir_tile = 0.  Tiles for one round of the waves
    the CUs hold, but never more than blocks / MIN_TILE of them, so that no tile is shorter than MIN_TILE blocks."""
    n_tiles = max(1, min(-(-RESIDENT[n_fft] * n_cu // n_sc), blocks // MIN_TILE))
    tile = -(-blocks // n_tiles)
    return tile, -(-blocks // tile)


def gpu_fir(nae, ctx, taps, n_fft, x, src_layout="i", dst_layout="i", shared=False, gap=0, offset=0, chan_pad=0):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_fir_block_f32; the frames behind each destination signal are checked untouched.
    gap: floats between the source's streams beyond n * ch; chan_pad: frames behind every planar channel, on both sides; offset: floats in
    front of the source's and the destination's base.  Whatever the source holds outside the signals is NaN, so a read there shows in the
    result; whatever the destination holds outside them is the sentinel, checked after the call."""
    n_streams, n, ch = x.shape
    xs = x[:1] if shared else x
    cs = n + chan_pad                                    # planar channel stride of the source
    ss = (n * ch if src_layout == "i" else cs * ch) + gap
    host = np.full(offset + xs.shape[0] * ss, np.nan, np.float32)
    body = host[offset:].reshape(xs.shape[0], ss)
    if src_layout == "i":
        body[:, :n * ch] = xs.reshape(xs.shape[0], n * ch)
    else:
        for c in range(ch):
            body[:, c * cs:c * cs + n] = xs[:, :, c]
    d_x = ctx.array(host)
    sss = 0 if shared else ss
    src = nae.Sig(d_x.at(offset), sss, 1, ch) if src_layout == "i" else nae.Sig(d_x.at(offset), sss, cs, 1)
    m = n + PAD + chan_pad
    d_y = ctx.array(np.full(offset + n_streams * m * ch, SENTINEL, np.float32))
    dst = nae.Sig(d_y.at(offset), m * ch, 1, ch) if dst_layout == "i" else nae.Sig(d_y.at(offset), m * ch, m, 1)
    ctx.fir_block(taps, src, n, ch, n_streams, dst, n_fft)
    out = d_y.download()
    d_x.free()
    d_y.free()
    assert np.all(out[:offset] == SENTINEL), "wrote in front of the destination"
    out = out[offset:]
    out = out.reshape(n_streams, m, ch) if dst_layout == "i" else out.reshape(n_streams, ch, m).transpose(0, 2, 1)
    assert np.all(out[:, n:, :] == SENTINEL), "wrote behind in_len"
    return np.ascontiguousarray(out[:, :n, :])


def ref_fir(ref, taps, n_fft, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([fir_ref.run(ref, taps, n_fft, s.reshape(-1), ch=x.shape[2]).reshape(s.shape) for s in x])


def ref_fir_flushed(ref, taps, n_fft, x):
    """what a flushed handle delivers for x[n, ch]: the statement on the input extended by len(taps) - 1 zero frames"""
    ext = np.concatenate([x, np.zeros((len(taps) - 1, x.shape[1]), np.float32)])
    return ref_fir(ref, taps, n_fft, ext[None])[0]


def fir_stream(nae, ctx, taps, n_fft, x, puts, device=False, handle=None):
    """x[n, ch] through a nae_fir handle (`handle`, or a new one): puts of the sizes in `puts` (the last one repeated) from the host or from
    device memory, a receive of everything available after every put, flush, the rest -> [n + len(taps) - 1, ch]"""
    n, ch = x.shape
    h = handle if handle is not None else nae.Fir(ctx, taps, ch, n_fft)
    d_x = ctx.array(x.reshape(-1)) if device else None
    try:
        parts, pos, i = [], 0, 0
        while pos < n:
            k = min(puts[min(i, len(puts) - 1)], n - pos)
            i += 1
            if device:
                h.put(d_x.at(pos * ch), k)
            else:
                h.put_host(x[pos:pos + k].reshape(-1))
            pos += k
            if h.available():
                parts.append(h.receive_host())
        h.flush()
        parts.append(h.receive_host())
        assert h.available() == 0
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
    return np.concatenate(parts).reshape(-1, ch)
