"""What the dynamics processor's GPU tests share (tests/test_gpu_dyn.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/dyn_ref/ref_dyn.c."""
import dyn_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/dyn_ref.Params -> the binding's DynParams"""
    return nae.DynParams(*dyn_ref.as_tuple(p))


def gpu_dyn(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_dyn_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.dyn_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def dyn_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_dyn handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has become
    available is floor((put - lookahead) / CHUNK) chunks, never negative."""
    h = nae.Dyn(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - p.lookahead, 0) // dyn_ref.CHUNK * dyn_ref.CHUNK, "whole chunks whose look-ahead is complete"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
