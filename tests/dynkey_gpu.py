"""What the keyed dynamics' GPU tests share (tests/test_gpu_dynkey.py): the block call bound to tests/block_gpu.py's views, with the key in a
view of its own, and the streaming handle's put loop (its puts are wider than its receives, so block_gpu.stream does not fit).  Every
comparison made with these is bit equality against tests/dynkey_ref/ref_dynkey.c."""
import numpy as np

import dyn_ref
import dynkey_ref
from block_gpu import STATE, view_call

KEY_PAD = 3    # NaN frames around every key signal


def lib_params(nae, p):
    """tests/dynkey_ref.Params -> the binding's DynKeyParams"""
    return nae.DynKeyParams.make(nae.DynParams(*dyn_ref.as_tuple(p.dyn)), p.key_ch, dynkey_ref.coef_of(p))


def key_view(nae, ctx, key, layout):
    """key[streams, n, kc] -> (device array, Sig): "i" interleaved, "p" planar, "s" one interleaved key for every stream (stream_stride = 0,
    key[0] is uploaded).  NaN stands in front of, between and behind the key's samples, so a read outside them shows in the result."""
    n_streams, n, kc = key.shape
    ks = key[:1] if layout == "s" else key
    m = n + KEY_PAD
    host = np.full(KEY_PAD + ks.shape[0] * m * kc, np.nan, np.float32)
    body = host[KEY_PAD:].reshape(ks.shape[0], m * kc)
    if layout == "p":
        for c in range(kc):
            body[:, c * m:c * m + n] = ks[:, :, c]
    else:
        body[:, :n * kc] = ks.reshape(ks.shape[0], n * kc)
    d = ctx.array(host)
    ss = 0 if layout == "s" else m * kc
    return d, (nae.Sig(d.at(KEY_PAD), ss, m, 1) if layout == "p" else nae.Sig(d.at(KEY_PAD), ss, 1, kc))


def gpu_dynkey(nae, ctx, p, x, key=None, *views, key_layout="i", **kw):
    """x[streams, n, ch], key[streams, n, key_ch] or None -> y[streams, n, ch] through nae_dynkey_block_f32: the signal in a view of
    block_gpu.view_call's (which checks the guard words around the destination), the key in key_view's"""
    d_key, ksig = (None, None) if key is None else key_view(nae, ctx, key, key_layout)
    try:
        return view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.dynkey_block(lib_params(nae, p), src, ksig, n, ch, n_streams, dst), x,
                         *views, **kw)
    finally:
        if d_key is not None:
            d_key.free()


def dynkey_stream(nae, ctx, p, x, key, puts, device=False, defer=False):
    """x[n, ch] and key[n, key_ch] (or None) through a nae_dynkey handle in frames of ch + key_ch floats -> [n, ch]: puts of the sizes in
    `puts` (the last one repeated) from the host or the device (a flag, or flags taken in turn), a receive of everything available after every
    put unless `defer`.  After every put what has become available is floor((put - lookahead) / CHUNK) chunks, never negative; the flush
    releases the rest, a second flush changes nothing, a put after it is NAE_ERR_STATE."""
    n, ch = x.shape
    frames = np.ascontiguousarray(x if key is None else np.concatenate([x, key], 1), np.float32)
    w = frames.shape[1]
    turn = tuple(device) if isinstance(device, (tuple, list)) else (device,)
    h = nae.DynKey(ctx, lib_params(nae, p), ch)
    d_x = ctx.array(frames.reshape(-1)) if any(turn) else None
    try:
        assert h.in_width == w
        parts, pos, i, taken = [], 0, 0, 0
        while pos < n:
            k = min(puts[min(i, len(puts) - 1)], n - pos)
            if turn[i % len(turn)]:
                h.put(d_x.at(pos * w), k)
            else:
                h.put_host(frames[pos:pos + k].reshape(-1))
            i += 1
            pos += k
            avail = h.available()
            assert taken + avail == max(pos - p.dyn.lookahead, 0) // dynkey_ref.CHUNK * dynkey_ref.CHUNK, "whole chunks whose look-ahead is complete"
            if avail and not defer:
                part = h.receive_host()
                assert part.size == avail * ch
                parts.append(part)
                taken += avail
        h.flush()
        h.flush()
        assert taken + h.available() == n, "the flush releases the rest"
        one = np.zeros(w, np.float32)
        assert h._fn("put_host")(h.h, one.ctypes.data, 1) == STATE, "put after flush: NAE_ERR_STATE"
        parts.append(h.receive_host())
        assert h.available() == 0
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
    return np.concatenate(parts).reshape(-1, ch)
