"""What the separation's GPU tests share (tests/test_gpu_hpss.py, tests/tools/fuzz_hpss.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/hpss_ref/ref_hpss.c."""
import hpss_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/hpss_ref.Params -> the binding's HpssParams"""
    return nae.HpssParams(*hpss_ref.as_tuple(p))


def gpu_hpss(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_hpss_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.hpss_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def hpss_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_hpss handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has
    become available is floor((put - (Tn + 3) H) / H) hop blocks, never negative."""
    h = nae.Hpss(ctx, lib_params(nae, p), x.shape[1])
    H, reach = p.n_fft // 4, (p.time_span + 3) * (p.n_fft // 4)

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - reach, 0) // H * H, "whole hop blocks with time_span + 3 blocks behind them"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
