"""What the FIR filter's GPU tests share (tests/test_gpu_fir.py, test_gpu_stream_long.py, test_gpu_multi_ctx.py, tests/tools/fuzz_fir.py): the
block call and the streaming handle bound to tests/block_gpu.py's views and put loop, the statement on streams, and a restatement of the
library's tile rule.  Every comparison made with these is bit equality against tests/fir_ref/ref_fir.c."""
import numpy as np

import fir_ref
from block_gpu import flushed, stream, view_call

WAVES = {512: 8, 1024: 8, 2048: 7, 4096: 3}        # Fir<N>::kWaves, waves (stream-channel x tile items) per workgroup
RESIDENT = {512: 16, 1024: 8, 2048: 7, 4096: 3}    # Fir<N>::kResident, waves a CU holds
MIN_TILE = 8                                       # NAE_FIR_MIN_TILE


def pick_tile(n_fft, blocks, n_sc, n_cu=256):
    """nae_pick_fir_tile restated: (blocks per tile, tiles per stream-channel) of a launch with fir_tile = 0.  Tiles for one round of the waves
    the CUs hold, but never more than blocks / MIN_TILE of them, so that no tile is shorter than MIN_TILE blocks."""
    n_tiles = max(1, min(-(-RESIDENT[n_fft] * n_cu // n_sc), blocks // MIN_TILE))
    tile = -(-blocks // n_tiles)
    return tile, -(-blocks // tile)


def gpu_fir(nae, ctx, taps, n_fft, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_fir_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.fir_block(taps, src, n, ch, n_streams, dst, n_fft), x, *views, **kw)


def ref_fir(ref, taps, n_fft, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([fir_ref.run(ref, taps, n_fft, s.reshape(-1), ch=x.shape[2]).reshape(s.shape) for s in x])


def ref_fir_flushed(ref, taps, n_fft, x):
    """what a flushed handle delivers for x[n, ch]: the statement on the input extended by len(taps) - 1 zero frames"""
    ext = np.concatenate([x, np.zeros((len(taps) - 1, x.shape[1]), np.float32)])
    return ref_fir(ref, taps, n_fft, ext[None])[0]


def fir_stream(nae, ctx, taps, n_fft, x, puts, device=False, handle=None):
    """x[n, ch] through a nae_fir handle (`handle`, or a new one) by block_gpu.stream -> [n + len(taps) - 1, ch]"""
    h = handle if handle is not None else nae.Fir(ctx, taps, x.shape[1], n_fft)
    return stream(h, ctx, x, puts, device, after_flush=flushed(h, len(x) + len(taps) - 1))
