"""What the vocoder's GPU tests share (tests/test_gpu_pv_*.py, tests/test_gpu_stretch_range.py): the two-tone and noise signals, a bit
comparison, the block call and the streaming handle.  The tone is also the CPU tests' (tests/test_pv_*_cpu.py)."""
import ctypes as C

import numpy as np

import orc

ENTRIES = ("ex", "n", "formant")          # nae_stretch_create_ex / _n / _formant


def tone(L, amp=(0.5, 0.25), f=(1000.0, 3300.0)):
    n = np.arange(L)
    return sum(a * np.sin(2 * np.pi * fr * n / 48000) for a, fr in zip(amp, f)).astype(np.float32)


def signal(kind, L, ch, seed=41, tonal=tone):
    """noise, or tonal(L) (the second channel at half level)"""
    if kind == "noise":
        return orc.fill_uniform(L * ch, seed)
    m = tonal(L)
    return np.stack([m, 0.5 * m], 1).reshape(-1).astype(np.float32) if ch == 2 else m


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def profiled(c, fn, *args, **kw):
    """(fn(*args, **kw), the set of kernels it launched on context c)"""
    c.prof_reset(); c.prof_enable(True)
    out = fn(*args, **kw)
    c.prof_enable(False)
    return out, set(c.prof_report())


def block(c, nae, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, n_streams=1, planar_in=False, planar_out=False):
    """the block call on x, [n_streams][L][ch] flattened -> interleaved [n_streams * out_len * ch], whatever the layouts on the device"""
    L = x.size // (ch * n_streams)
    pl = c.stretch_plan(rate, pitch, L, n_fft)
    flat = np.ascontiguousarray(x.reshape(n_streams, L, ch).transpose(0, 2, 1)).reshape(-1) if planar_in else x
    d_x, d_o = c.array(np.ascontiguousarray(flat, np.float32)), c.empty(max(1, n_streams * pl.out_len * ch))
    src = nae.Sig.planar(d_x.ptr, L, ch) if planar_in else nae.Sig.interleaved(d_x.ptr, L, ch)
    dst = nae.Sig.planar(d_o.ptr, pl.out_len, ch) if planar_out else nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)
    c.stretch_block(rate, pitch, src, L, ch, n_streams, dst, phase_lock=lock, n_fft=n_fft, formant=lifter)
    out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    if planar_out:
        out = np.ascontiguousarray(out.reshape(n_streams, ch, pl.out_len).transpose(0, 2, 1)).reshape(-1)
    return out


def stream(c, x, ch, rate, pitch, put_sizes, entry, n_fft=1024, flags=0, lifter=0, sample_rate=48000, repeat_last=False,
           device_put=False):
    """the streaming handle made by nae_stretch_create_<entry>: puts of put_sizes (cycled, or with repeat_last the last one repeated) from
    the host, or from device memory with device_put; a receive after every put, then flush and receive: the whole output, interleaved"""
    lib = c.lib
    L = x.size // ch
    h = C.c_void_p()
    if entry == "ex":
        rc = lib.nae_stretch_create_ex(c.h, sample_rate, ch, rate, pitch, flags, C.byref(h))
    elif entry == "n":
        rc = lib.nae_stretch_create_n(c.h, sample_rate, ch, rate, pitch, flags, n_fft, C.byref(h))
    else:
        assert entry == "formant", entry
        rc = lib.nae_stretch_create_formant(c.h, sample_rate, ch, rate, pitch, flags, n_fft, lifter, C.byref(h))
    assert rc == 0, rc
    outs, pos, i = [], 0, 0
    d_x = c.array(x) if device_put else None

    def drain():
        n = lib.nae_stretch_available(h)
        if n:
            buf = np.empty(n * ch, np.float32)
            got = C.c_size_t()
            assert lib.nae_stretch_receive_host(h, buf.ctypes.data, n, C.byref(got)) == 0
            outs.append(buf[: got.value * ch])

    while pos < L:
        size = put_sizes[-1] if repeat_last and i >= len(put_sizes) else put_sizes[i % len(put_sizes)]
        n = min(size, L - pos)
        i += 1
        if device_put:
            assert lib.nae_stretch_put(h, d_x.at(pos * ch), n) == 0
        else:
            chunk = np.ascontiguousarray(x[pos * ch:(pos + n) * ch])
            assert lib.nae_stretch_put_host(h, chunk.ctypes.data, n) == 0
        pos += n
        drain()
    assert lib.nae_stretch_flush(h) == 0
    drain()
    assert lib.nae_stretch_destroy(h) == 0
    if d_x is not None:
        d_x.free()
    return np.concatenate(outs) if outs else np.zeros(0, np.float32)
