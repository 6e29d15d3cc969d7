"""What the saturation's GPU tests share (tests/test_gpu_sat.py, tests/tools/fuzz_sat.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/sat_ref/ref_sat.c."""
import ctypes as C

import sat_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/sat_ref.Params -> the binding's SatParams (the records have one layout: tests/test_sat_cpu.py)"""
    lp = nae.SatParams()
    C.memmove(C.byref(lp), C.byref(p), C.sizeof(lp))
    return lp


def gpu_sat(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_sat_block_f32 in a view of block_gpu.view_call's"""
    lp = lib_params(nae, p)
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.sat_block(lp, src, n, ch, n_streams, dst), x, *views, **kw)


def sat_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_sat handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n + D, ch].  What is available is whole
    chunks of what was put until the flush, which releases the rest and the latency's tail."""
    h = nae.Sat(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == pos // sat_ref.CHUNK * sat_ref.CHUNK, "whole chunks come out as they fill"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x) + sat_ref.latency(p.oversample)), **drive)
