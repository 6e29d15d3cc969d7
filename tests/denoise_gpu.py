"""What the spectral gate's GPU tests share (tests/test_gpu_denoise.py): the profile entry, the block call and the streaming handle bound to
tests/block_gpu.py's views and put loop.  Every comparison made with these is bit equality against tests/denoise_ref/ref_denoise.c."""
import numpy as np

import denoise_ref
from block_gpu import flushed, stream, view_call


def lib_params(nae, p):
    """tests/denoise_ref.Params -> the binding's DenoiseParams"""
    return nae.DenoiseParams(*denoise_ref.as_tuple(p))


def gpu_denoise(nae, ctx, p, profile, x, *views, **kw):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_denoise_block_f32 in a view of block_gpu.view_call's; profile[1 or ch, bins]"""
    profile = np.ascontiguousarray(profile, np.float32).reshape(-1, p.n_fft // 2 + 1)
    d_p = ctx.array(profile.reshape(-1))
    try:
        return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.denoise_block(lib_params(nae, p), d_p.ptr, profile.shape[0], src, n, ch,
                                                                                        n_streams, dst), x, *views, **kw)
    finally:
        d_p.free()


def gpu_profile(nae, ctx, n_fft, x, layout="i"):
    """x[len, ch] -> [ch, n_fft / 2 + 1] through nae_denoise_profile_f32; guard words around the result must stay"""
    n, ch = x.shape
    K = n_fft // 2 + 1
    host = np.ascontiguousarray(x if layout == "i" else x.T, np.float32).reshape(-1)
    d_x = ctx.array(host)
    d_p = ctx.array(np.full(ch * K + 16, -12345.0, np.float32))
    try:
        src = nae.Sig(d_x.ptr, 0, 1, ch) if layout == "i" else nae.Sig(d_x.ptr, 0, n, 1)
        ctx.denoise_profile(n_fft, src, n, ch, d_p.at(8))
        out = d_p.download()
    finally:
        d_x.free()
        d_p.free()
    assert np.all(out[:8] == -12345.0) and np.all(out[8 + ch * K:] == -12345.0), "wrote outside the profile"
    return out[8:8 + ch * K].reshape(ch, K).copy()


def denoise_stream(nae, ctx, p, profile, x, puts, device=False, **drive):
    """x[n, ch] through a nae_denoise handle by block_gpu.stream (drive: its d_out, defer and piece) -> [n, ch].  Before the flush what has
    become available is floor((put - (Tn + 3) H) / H) hop blocks, never negative."""
    profile = np.ascontiguousarray(profile, np.float32).reshape(-1, p.n_fft // 2 + 1)
    d_p = ctx.array(profile.reshape(-1))
    h = nae.Denoise(ctx, lib_params(nae, p), d_p.ptr, profile.shape[0], x.shape[1])
    ctx.sync()
    d_p.free()                                             # the handle has its own copy
    H, reach = p.n_fft // 4, (p.time_smooth + 3) * (p.n_fft // 4)

    def on_put(pos, taken, avail):
        assert taken + avail == max(pos - reach, 0) // H * H, "whole hop blocks with time_smooth + 3 blocks behind them"
    return stream(h, ctx, x, puts, device, on_put, flushed(h, len(x)), **drive)
