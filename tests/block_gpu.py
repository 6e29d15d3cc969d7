"""What the GPU tests of the block entries and their streaming handles share (FIR filter, long convolution, equalizer, dynamics: tests/fir_gpu.py,
eq_gpu.py, dyn_gpu.py and tests/test_gpu_conv.py bind their entries to it): the views every block entry is called in, a bit view, the noise,
the CPU statements built once per process, `view_call` (a block call with guard words around the signals) and `stream` (the put loop of a
handle); for the large batches of tests/test_gpu_batch.py, `each_stream` (a statement on every stream) and `mismatch` (which streams differ).
tests/test_block_harness_cpu.py pins, without a GPU, that the guards catch what they are there to catch."""
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

PAD = 8        # frames behind every destination signal that must stay untouched
SENTINEL = np.float32(-12345.0)
# (channels, streams, source layout, destination layout, shared source): interleaved and planar views on both sides, stream_stride = 0
CONFIGS = ((1, 1, "i", "i", False), (2, 1, "i", "i", False), (1, 3, "p", "p", False), (2, 3, "p", "p", False),
           (2, 3, "i", "p", False), (2, 1, "p", "i", False), (2, 3, "i", "i", True), (1, 3, "p", "p", True))
STATE = -5     # NAE_ERR_STATE

_statements = {}


def statement(ref_module):
    """the CPU statement's library of tests/fir_ref.py, conv_ref.py, eq_ref.py or dyn_ref.py, compiled once per process"""
    if ref_module not in _statements:
        tmp = tempfile.TemporaryDirectory(prefix="ref_statement")
        _statements[ref_module] = (ref_module.build(tmp.name), tmp)
    return _statements[ref_module][0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def each_stream(fn, n_streams):
    """np.stack of fn(0) ... fn(n_streams - 1): a statement on every stream of a large batch, on a few threads.  The statements are C calls
    through ctypes, which releases the interpreter's lock around them, and they keep no state between calls, so the result does not depend
    on the threads; fn(0) runs first and alone."""
    if n_streams < 16:
        return np.stack([fn(i) for i in range(n_streams)])
    first = fn(0)
    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack([first] + list(pool.map(fn, range(1, n_streams))))


def mismatch(got, want, first=8):
    """"" where got[streams, n, ch] has want's bits; else a message for an assertion on a large batch: how many streams differ, and the first
    few (stream, channel, first differing sample, differing samples) of them: a pattern in the indices is the diagnosis"""
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = bits(got) != bits(want)
    pairs = np.argwhere(diff.any(axis=1))
    if len(pairs) == 0:
        return ""
    where = [(int(s), int(c), int(np.argmax(diff[s, :, c])), int(diff[s, :, c].sum())) for s, c in pairs[:first]]
    return (f"{len(np.unique(pairs[:, 0]))} of {got.shape[0]} streams differ ({len(pairs)} stream-channels); "
            f"first (stream, channel, first sample, samples): {where}")


def noise(rng, n_streams, n, ch, shared=False):
    x = rng.uniform(-1, 1, (n_streams, n, ch)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def view_call(nae, ctx, call, x, src_layout="i", dst_layout="i", shared=False, gap=0, offset=0, chan_pad=0):
    """x[streams, n, ch] -> y[streams, n, ch] through call(src_sig, n, ch, n_streams, dst_sig), a block entry; the frames behind each
    destination signal are checked untouched.  gap: floats between the source's streams beyond n * ch; chan_pad: frames behind every planar
    channel, on both sides; offset: floats in front of the source's and the destination's base (an odd one gives a base that is 4-byte
    aligned only).  Whatever the source holds outside the signals is NaN, so a read there shows in the result; whatever the destination
    holds outside them is the sentinel, checked after the call."""
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
    call(src, n, ch, n_streams, dst)
    out = d_y.download()
    d_x.free()
    d_y.free()
    assert np.all(out[:offset] == SENTINEL), "wrote in front of the destination"
    out = out[offset:]
    out = out.reshape(n_streams, m, ch) if dst_layout == "i" else out.reshape(n_streams, ch, m).transpose(0, 2, 1)
    assert np.all(out[:, n:, :] == SENTINEL), "wrote behind in_len"
    return np.ascontiguousarray(out[:, :n, :])


def stream(h, ctx, x, puts, device=False, on_put=None, after_flush=None, d_out=None, defer=False, piece=None):
    """x[n, ch] through the handle h, which is closed at the end: puts of the sizes in `puts` (the last one repeated) from the host or from
    device memory (device: one flag, or a sequence of flags taken in turn, put after put), a receive of everything available after every put
    (into the device array d_out, if given, else into host memory), flush, the rest -> [frames out, ch].  defer: nothing is received before
    the flush, so the handle's output grows while all of it is live.  piece: a receive takes at most that many frames, and is repeated
    until nothing is left.  on_put(pos, taken, avail) after every put, with the frames put and received so far and those available;
    after_flush(taken) between the flush and the last receive."""
    n, ch = x.shape
    turn = tuple(device) if isinstance(device, (tuple, list)) else (device,)
    d_x = ctx.array(x.reshape(-1)) if any(turn) else None
    try:
        parts, pos, i, taken = [], 0, 0, 0

        def take():
            left = h.available()
            while True:
                k = left if piece is None else min(piece, left)
                if d_out is None:
                    part = h.receive_host() if piece is None else h.receive_host(k)
                else:
                    got = h.receive(d_out.ptr, k)
                    part = d_out.download()[:got * ch].copy()
                assert part.size == k * ch, "a receive delivers what was asked for and is available"
                parts.append(part)
                left -= k
                if left == 0:
                    break
        while pos < n:
            k = min(puts[min(i, len(puts) - 1)], n - pos)
            if turn[i % len(turn)]:
                h.put(d_x.at(pos * ch), k)
            else:
                h.put_host(x[pos:pos + k].reshape(-1))
            i += 1
            pos += k
            avail = h.available()
            if on_put:
                on_put(pos, taken, avail)
            if avail and not defer:
                take()
                taken += avail
        h.flush()
        if after_flush:
            after_flush(taken)
        take()
        assert h.available() == 0
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
    return np.concatenate(parts).reshape(-1, ch)


def flushed(h, out_len):
    """an after_flush for the library's handles: a second flush changes nothing, out_len frames come out in all, a put is NAE_ERR_STATE"""
    def check(taken):
        h.flush()
        assert taken + h.available() == out_len, "the flush releases the rest: the length the header states"
        one = np.zeros(h.ch, np.float32)
        assert h._fn("put_host")(h.h, one.ctypes.data, 1) == STATE, "put after flush: NAE_ERR_STATE"
    return check
