"""What the multiband compressor's GPU tests share (tests/test_gpu_mb.py, tests/tools/fuzz_mb.py): the block call and the streaming handle
bound to tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/mb_ref/ref_mb.c."""
import mb_ref
from block_gpu import flushed, stream, view_call
from mb_ref import lib_params  # noqa: F401 — the tests take it from here, as they take the other nodes'


def gpu_mb(nae, ctx, p, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_mb_block_f32 in a view of block_gpu.view_call's"""
    return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.mb_block(lib_params(nae, p), src, n, ch, n_streams, dst), x, *views, **kw)


def mb_stream(nae, ctx, p, x, puts, device=False, **drive):
    """x[n, ch] through a nae_mb handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has become
    available is floor((put - lookahead) / CHUNK) chunks, never negative."""
    h = nae.Multiband(ctx, lib_params(nae, p), x.shape[1])
    la = p.band[0].lookahead

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - la, 0) // mb_ref.CHUNK * mb_ref.CHUNK, "whole chunks whose look-ahead is complete"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)


class debug_keys:
    """with debug_keys(ctx, mb_slab=1, mb_group=2): the keys for the block, 0 again behind it"""

    def __init__(self, ctx, **keys):
        self.ctx, self.keys = ctx, keys

    def __enter__(self):
        for k, v in self.keys.items():
            self.ctx.debug_set(k, v)

    def __exit__(self, *exc):
        for k in self.keys:
            self.ctx.debug_set(k, 0)
