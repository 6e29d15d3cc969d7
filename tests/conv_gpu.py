"""What the long convolution's GPU tests share (tests/test_gpu_conv.py, tests/tools/fuzz_effects.py): the block call and the streaming handle
bound to tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/conv_ref/ref_conv.c."""
from block_gpu import flushed, stream, view_call


def gpu_conv(nae, ctx, taps, n_fft, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_conv_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.conv_block(taps, src, n, ch, n_streams, dst, n_fft), x, *views, **kw)


def conv_stream(nae, ctx, taps, n_fft, x, puts, device=False):
    """x[n, ch] through a nae_conv handle by block_gpu.stream, received into device memory when the puts come from it"""
    n, ch = x.shape
    h = nae.Conv(ctx, taps, ch, n_fft)
    d_y = ctx.empty((n + taps.shape[-1]) * ch) if device else None
    try:
        return stream(h, ctx, x, puts, device, after_flush=flushed(h, n + taps.shape[-1] - 1), d_out=d_y)
    finally:
        if d_y is not None:
            d_y.free()
