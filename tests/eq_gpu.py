"""What the equalizer's GPU tests share (tests/test_gpu_eq.py): the CPU statement built once per process, a bit view, the block call in every
view with guard words around the signals, and the streaming handle.  Every comparison made with these is bit equality against
tests/eq_ref/ref_eq.c."""
import tempfile

import numpy as np

import eq_ref

PAD = 8        # frames behind every destination signal that must stay untouched
SENTINEL = np.float32(-12345.0)
# (channels, streams, source layout, destination layout, shared source): interleaved and planar views on both sides, stream_stride = 0
CONFIGS = ((1, 1, "i", "i", False), (2, 1, "i", "i", False), (1, 3, "p", "p", False), (2, 3, "p", "p", False),
           (2, 3, "i", "p", False), (2, 1, "p", "i", False), (2, 3, "i", "i", True), (1, 3, "p", "p", True))

_statement = None


def statement():
    """the CPU statement's library, compiled once per process"""
    global _statement
    if _statement is None:
        tmp = tempfile.TemporaryDirectory(prefix="ref_eq_gpu")
        _statement = (eq_ref.build(tmp.name), tmp)
    return _statement[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(rng, n_streams, n, ch, shared=False):
    x = rng.uniform(-1, 1, (n_streams, n, ch)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def gpu_eq(nae, ctx, coef, x, src_layout="i", dst_layout="i", shared=False, gap=0, offset=0, chan_pad=0):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_eq_block_f32; the frames behind each destination signal are checked untouched.
    gap: floats between the source's streams beyond n * ch; chan_pad: frames behind every planar channel, on both sides; offset: floats in
    front of the source's and the destination's base (an odd one gives a base that is 4-byte aligned only).  Whatever the source holds outside
    the signals is NaN, so a read there shows in the result; whatever the destination holds outside them is the sentinel, checked after the
    call."""
    n_streams, n, ch = x.shape
    xs = x[:1] if shared else x
    cs = n + chan_pad                                    # planar channel stride of the source
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
    ctx.eq_block(coef, src, n, ch, n_streams, dst)
    out = d_y.download()
    d_x.free()
    d_y.free()
    assert np.all(out[:offset] == SENTINEL), "wrote in front of the destination"
    out = out[offset:]
    out = out.reshape(n_streams, m, ch) if dst_layout == "i" else out.reshape(n_streams, ch, m).transpose(0, 2, 1)
    assert np.all(out[:, n:, :] == SENTINEL), "wrote behind in_len"
    return np.ascontiguousarray(out[:, :n, :])


def eq_stream(nae, ctx, coef, x, puts, device=False):
    """x[n, ch] through a nae_eq handle: puts of the sizes in `puts` (the last one repeated) from the host or from device memory, a receive of
    everything available after every put, flush, the rest -> [n, ch].  What is available never exceeds what was put, and is whole chunks
    until the flush."""
    n, ch = x.shape
    h = nae.Eq(ctx, coef, ch)
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
            assert taken + avail <= pos, "more available than was put"
            assert taken + avail == pos // eq_ref.CHUNK * eq_ref.CHUNK, "whole chunks come out as they fill"
            if avail:
                parts.append(h.receive_host())
                taken += avail
        h.flush()
        h.flush()                                          # a second flush changes nothing
        assert taken + h.available() == n, "the flush releases the partial last chunk: in_len frames in all"
        parts.append(h.receive_host())
        assert h.available() == 0
        one = np.zeros(ch, np.float32)
        assert ctx.lib.nae_eq_put_host(h.h, one.ctypes.data, 1) == -5, "put after flush: NAE_ERR_STATE, as the other handles"
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
    return np.concatenate(parts).reshape(-1, ch)
