"""What the dynamics processor's GPU tests share (tests/test_gpu_dyn.py): the CPU statement built once per process, a bit view, the block call
in every view with NaN outside the source signals and a sentinel outside the destination, and the streaming handle.  Every comparison made
with these is bit equality against tests/dyn_ref/ref_dyn.c."""
import tempfile

import numpy as np

import dyn_ref
from eq_gpu import CONFIGS, PAD, SENTINEL, bits, noise  # noqa: F401 — the views and helpers of the equalizer's tests

_statement = None


def statement():
    """the CPU statement's library, compiled once per process"""
    global _statement
    if _statement is None:
        tmp = tempfile.TemporaryDirectory(prefix="ref_dyn_gpu")
        _statement = (dyn_ref.build(tmp.name), tmp)
    return _statement[0]


def lib_params(nae, p):
    """tests/dyn_ref.Params -> the binding's DynParams"""
    return nae.DynParams(*dyn_ref.as_tuple(p))


def gpu_dyn(nae, ctx, p, x, src_layout="i", dst_layout="i", shared=False, gap=0, offset=0, chan_pad=0):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_dyn_block_f32; arguments as eq_gpu.gpu_eq's.  Whatever the source holds outside the
    signals is NaN, so a read there shows in the result; whatever the destination holds outside them is the sentinel, checked after the call."""
    n_streams, n, ch = x.shape
    xs = x[:1] if shared else x
    cs = n + chan_pad
    ss = (n * ch if src_layout == "i" else cs * ch) + gap
    host = np.full(offset + xs.shape[0] * ss, np.nan, np.float32)
    body = host[offset:].reshape(xs.shape[0], ss)
    if src_layout == "i":
        body[:, :n * ch] = xs.reshape(xs.shape[0], n * ch)
    else:
        for c in range(ch):
            body[:, c * cs:c * cs + n] = xs[:, :, c]
    d_x = ctx.array(host)
    sss = 0 if shared else ss
    src = nae.Sig(d_x.at(offset), sss, 1, ch) if src_layout == "i" else nae.Sig(d_x.at(offset), sss, cs, 1)
    m = n + PAD + chan_pad
    d_y = ctx.array(np.full(offset + n_streams * m * ch, SENTINEL, np.float32))
    dst = nae.Sig(d_y.at(offset), m * ch, 1, ch) if dst_layout == "i" else nae.Sig(d_y.at(offset), m * ch, m, 1)
    ctx.dyn_block(lib_params(nae, p), src, n, ch, n_streams, dst)
    out = d_y.download()
    d_x.free()
    d_y.free()
    assert np.all(out[:offset] == SENTINEL), "wrote in front of the destination"
    out = out[offset:]
    out = out.reshape(n_streams, m, ch) if dst_layout == "i" else out.reshape(n_streams, ch, m).transpose(0, 2, 1)
    assert np.all(out[:, n:, :] == SENTINEL), "wrote behind in_len"
    return np.ascontiguousarray(out[:, :n, :])


def dyn_stream(nae, ctx, p, x, puts, device=False):
    """x[n, ch] through a nae_dyn handle: puts of the sizes in `puts` (the last one repeated) from the host or from device memory, a receive
    of everything available after every put, flush, the rest -> [n, ch].  Before the flush what has become available is
    floor((put - lookahead) / CHUNK) chunks, never negative."""
    n, ch = x.shape
    h = nae.Dyn(ctx, lib_params(nae, p), ch)
    d_x = ctx.array(x.reshape(-1)) if device else None
    try:
        parts, pos, i, taken = [], 0, 0, 0
        while pos < n:
            k = min(puts[min(i, len(puts) - 1)], n - pos)
            i += 1
            if device:
                h.put(d_x.at(pos * ch), k)
            else:
                h.put_host(x[pos:pos + k].reshape(-1))
            pos += k
            avail = h.available()
            assert taken + avail == max(pos - p.lookahead, 0) // dyn_ref.CHUNK * dyn_ref.CHUNK, "whole chunks whose look-ahead is complete"
            if avail:
                parts.append(h.receive_host())
                taken += avail
        h.flush()
        h.flush()                                          # a second flush changes nothing
        assert taken + h.available() == n, "the flush releases the rest: in_len frames in all"
        parts.append(h.receive_host())
        assert h.available() == 0
        one = np.zeros(ch, np.float32)
        assert ctx.lib.nae_dyn_put_host(h.h, one.ctypes.data, 1) == -5, "put after flush: NAE_ERR_STATE, as the other handles"
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
    return np.concatenate(parts).reshape(-1, ch)
