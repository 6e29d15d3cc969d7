"""What the echo's GPU tests share (tests/test_gpu_echo.py): the block call and the streaming handle bound to tests/block_gpu.py's views and
put loop.  Every comparison made with these is bit equality against tests/echo_ref/ref_echo.c."""
import echo_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/echo_ref.Params -> the binding's EchoParams"""
    return nae.EchoParams.make((p.delay[0], p.delay[1]), p.feedback, p.cross, p.wet, p.dry, echo_ref.coef_of(p))


def gpu_echo(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_echo_block_f32 in a view of block_gpu.view_call's"""
    lp = lib_params(nae, p)
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.echo_block(lp, src, n, ch, n_streams, dst), x, *views, **kw)


def echo_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_echo handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  What is available never exceeds
    what was put, and is whole chunks until the flush."""
    h = nae.Echo(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == pos // echo_ref.CHUNK * echo_ref.CHUNK, "whole chunks come out as they fill"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
