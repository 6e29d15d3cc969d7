"""What the modulated delay's GPU tests share (tests/test_gpu_mod.py): the block call and the streaming handle
bound to tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/mod_ref/ref_mod.c."""
import ctypes as C

import mod_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/mod_ref.Params -> the binding's ModParams (the records have one layout: tests/test_mod_cpu.py)"""
    lp = nae.ModParams()
    C.memmove(C.byref(lp), C.byref(p), C.sizeof(lp))
    return lp


def gpu_mod(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_mod_block_f32 in a view of block_gpu.view_call's"""
    lp = lib_params(nae, p)
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.mod_block(lp, src, n, ch, n_streams, dst), x, *views, **kw)


def mod_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_mod handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  What is available never exceeds
    what was put, and is whole chunks until the flush."""
    h = nae.Mod(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == pos // mod_ref.CHUNK * mod_ref.CHUNK, "whole chunks come out as they fill"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
