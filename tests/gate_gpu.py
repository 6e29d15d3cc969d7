"""What the gate's GPU tests share (tests/test_gpu_gate.py, tests/tools/fuzz_gate.py): the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/gate_ref/ref_gate.c."""
import gate_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/gate_ref.Params -> the binding's GateParams"""
    return nae.GateParams(*gate_ref.as_tuple(p))


def gpu_gate(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_gate_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.gate_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def gate_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_gate handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has become
    available is floor((put - lookahead) / CHUNK) chunks, never negative."""
    h = nae.Gate(ctx, lib_params(nae, p), x.shape[1])

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - p.lookahead, 0) // gate_ref.CHUNK * gate_ref.CHUNK, "whole chunks whose look-ahead is complete"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
