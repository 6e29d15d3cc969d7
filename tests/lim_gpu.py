"""What the limiter's GPU tests share (tests/test_gpu_lim.py, tests/tools/fuzz_lim.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/lim_ref/ref_lim.c."""
import lim_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/lim_ref.Params -> the binding's LimParams"""
    return nae.LimParams(*lim_ref.as_tuple(p))


def gpu_lim(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_lim_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.lim_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def lim_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_lim handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has become
    available is floor((put - lookahead - D) / CHUNK) chunks, never negative."""
    h = nae.Limiter(ctx, lib_params(nae, p), x.shape[1])
    wait = p.lookahead + lim_ref.reach(p)

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - wait, 0) // lim_ref.CHUNK * lim_ref.CHUNK, "whole chunks whose look-ahead and reach are complete"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
