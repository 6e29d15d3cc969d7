"""What the dither's GPU tests share (tests/test_gpu_dither.py, tests/tools/fuzz_dither.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/dither_ref/ref_dither.c."""
import dither_ref
from block_gpu import flushed, mismatch, stream, view_call


def lib_params(nae, p):
    """tests/dither_ref.Params -> the binding's DitherParams"""
    return nae.DitherParams.from_buffer_copy(bytes(p))


def gpu_dither(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_dither_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.dither_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def same(nae, ctx, L, p, x, *views, shared=False, **kw):
    """"" where the block call on x[streams, n, ch] has the statement's bits, stream s under its own key (block_gpu.mismatch's message else)"""
    got = gpu_dither(nae, ctx, p, x, *views, shared=shared, **kw)
    return mismatch(got, dither_ref.run_streams(L, p, x, shared))


def dither_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_dither handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  The handle has no latency:
    after every put all frames put so far have been available."""
    h = nae.Dither(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == pos, "every frame put is available after that put"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
