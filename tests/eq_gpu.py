"""What the equalizer's GPU tests share (tests/test_gpu_eq.py): the block call and the streaming handle bound to tests/block_gpu.py's views
and put loop.  Every comparison made with these is bit equality against tests/eq_ref/ref_eq.c."""
import eq_ref
from block_gpu import flushed, stream, view_call


def gpu_eq(nae, ctx, coef, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_eq_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.eq_block(coef, src, n, ch, n_streams, dst), x, *views, **kw)


def eq_stream(nae, ctx, coef, x, puts, device=False, **drive):
    """x[n, ch] through a nae_eq handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  What is available never exceeds what
    was put, and is whole chunks until the flush."""
    h = nae.Eq(ctx, coef, x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail <= pos, "more available than was put"
        assert taken + avail == pos // eq_ref.CHUNK * eq_ref.CHUNK, "whole chunks come out as they fill"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
