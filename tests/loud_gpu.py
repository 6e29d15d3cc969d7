"""What the loudness meter's GPU tests share (tests/test_gpu_loud.py): the block entries bound to tests/block_gpu.py's views, a record buffer
between guard bytes, and the put loop of the measuring handle.  Every comparison made with these is bit equality against
tests/loud_ref/ref_loud.c: the records field by field, doubles by their 64 bits."""
import ctypes as C

import numpy as np

import loud_ref
from block_gpu import SENTINEL, view_call

GUARD = 64                      # bytes in front of and behind the records that must stay untouched
GUARD_BYTE = 0xA5


def with_records(nae, ctx, n_streams, run):
    """run(results_ptr) with room for n_streams nae_loud_result records between guard bytes -> the records"""
    size = C.sizeof(nae.LoudResult)
    d = ctx.array(np.full(2 * GUARD + n_streams * size, GUARD_BYTE, np.uint8))
    try:
        run(d.at(GUARD))
        raw = d.download()
    finally:
        d.free()
    assert np.all(raw[:GUARD] == GUARD_BYTE), "wrote in front of the records"
    assert np.all(raw[GUARD + n_streams * size:] == GUARD_BYTE), "wrote behind the records"
    return [nae.LoudResult.from_buffer_copy(raw[GUARD + i * size:GUARD + (i + 1) * size].tobytes()) for i in range(n_streams)]


def gpu_measure(nae, ctx, params, x, *views, **kw):
    """x[streams, n, ch] -> the records of nae_loud_measure_f32 in a view of block_gpu.view_call's; the destination it is given stays untouched"""
    out = {}

    def run(ptr):
        out["y"] = view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.loud_measure(params, src, n, ch, n_streams, ptr), x, *views, **kw)
    records = with_records(nae, ctx, x.shape[0], run)
    assert np.all(out["y"] == SENTINEL), "measuring writes no samples"
    return records


def gpu_normalize(nae, ctx, params, x, *views, records=True, **kw):
    """x[streams, n, ch] -> (y[streams, n, ch], records) of nae_loud_normalize_f32; records=False: the library keeps them (a null pointer)"""
    out = {}

    def run(ptr):
        out["y"] = view_call(nae, ctx, lambda src, n, ch, n_streams, dst: ctx.loud_normalize(params, src, n, ch, n_streams, dst, ptr if records else 0),
                             x, *views, **kw)
    got = with_records(nae, ctx, x.shape[0], run)
    if not records:
        assert all(bytes(r) == bytes([GUARD_BYTE]) * C.sizeof(nae.LoudResult) for r in got), "no record buffer given, none written"
    return out["y"], got


def gpu_measure_apply(nae, ctx, params, x, *views, **kw):
    """x[streams, n, ch] -> (y, records): nae_loud_measure_f32, then nae_loud_apply_f32 as an entry of its own with the records it left"""
    out = {}

    def both(ptr):
        def call(src, n, ch, n_streams, dst):
            ctx.loud_measure(params, src, n, ch, n_streams, ptr)
            ctx.loud_apply(ptr, src, n, ch, n_streams, dst)
        out["y"] = view_call(nae, ctx, call, x, *views, **kw)
    records = with_records(nae, ctx, x.shape[0], both)
    return out["y"], records


def same_record(got, want):
    """every field, bit for bit (doubles by their 64 bits)"""
    g, w = loud_ref.record_fields(got), loud_ref.record_fields(want)
    assert g == w, {k: (g[k], w[k]) for k in g if g[k] != w[k]}


def loud_stream(nae, ctx, params, x, puts, device=False):
    """x[n, ch] through a nae_loud handle: puts of the sizes in `puts` (the last one repeated), from the host or from device memory (device: one
    flag, or a sequence of flags taken in turn) -> the record.  Before the flush the record is NAE_ERR_STATE; behind it a put is."""
    n, ch = x.shape
    turn = tuple(device) if isinstance(device, (tuple, list)) else (device,)
    d_x = ctx.array(x.reshape(-1)) if any(turn) else None
    h = nae.Loud(ctx, params, ch)
    try:
        pos = i = 0
        while pos < n:
            k = min(puts[min(i, len(puts) - 1)], n - pos)
            if turn[i % len(turn)]:
                h.put(d_x.at(pos * ch), k)
            else:
                h.put_host(x[pos:pos + k].reshape(-1))
            i += 1
            pos += k
        probe = nae.LoudResult()
        assert h._fn("get_result")(h.h, C.byref(probe)) == -5, "the record before the flush: NAE_ERR_STATE"
        h.flush()
        h.flush()
        one = np.zeros(ch, np.float32)
        assert h._fn("put_host")(h.h, one.ctypes.data, 1) == -5, "put after flush: NAE_ERR_STATE"
        return h.result()
    finally:
        h.close()
        if d_x is not None:
            d_x.free()
