"""Long streams through every streaming handle (nae_stretch, nae_wsola, nae_swr, nae_spectrum, nae_fir and the block-handle family nae_eq,
nae_dyn, nae_dynkey, nae_echo, nae_conv, nae_denoise): 300 000+ frames in an uneven cycle of put sizes, with receives that take
everything, part of what is available or nothing.  Every device FIFO of the handles grows several times and is compacted many times; the
output equals the block call, the oracle or the CPU statement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import conv_ref
import denoise_ref
import dyn_ref
import dynkey_ref
import echo_ref
import eq_ref
import fir_ref
import orc
import pv_ref
from block_gpu import statement
from denoise_gpu import lib_params as denoise_params
from dyn_gpu import lib_params as dyn_params
from dynkey_gpu import lib_params as dynkey_params
from echo_gpu import lib_params as echo_params
from eq_gpu import gpu_eq
from fir_gpu import gpu_fir
from pv_gpu import block, same_bits
from test_gpu_spectrum_sizes import bins, gpu_ex

pytestmark = pytest.mark.gpu

L = 400_000
PUTS = [1, 37, 1152, 4096, 20000, 1, 37, 1152, 4096, 20000, 90001]


def f32(v):
    return float(np.float32(v))


def schedule(L, put_sizes=PUTS):
    """(first frame, frames) of every put, and how much of what is available the receive after it takes"""
    pos, i = 0, 0
    while pos < L:
        n = min(put_sizes[i % len(put_sizes)], L - pos)
        yield pos, n, (None, 0.5, None, 1.0)[i % 4]       # nothing, about half, nothing, everything
        pos += n
        i += 1


def part(avail, share):
    return 0 if share is None else (avail if share == 1.0 else avail // 2 + 1 if avail else 0)


def drive(lib, h, prefix, x, ch, in_ch=None):
    """put_host / available / receive_host / flush / receive everything of a handle with these entries (nae_stretch, nae_wsola, nae_fir, the
    block handles); in_ch: the floats of a put frame where they are not the ch of a received one (nae_dynkey's carry the key)"""
    in_ch = ch if in_ch is None else in_ch
    put, available, receive = (getattr(lib, f"nae_{prefix}_{f}") for f in ("put_host", "available", "receive_host"))
    outs, got = [], C.c_size_t()

    def take(n):
        if n:
            buf = np.empty(n * ch, np.float32)
            assert receive(h, buf.ctypes.data, n, C.byref(got)) == 0
            assert got.value == n
            outs.append(buf)

    for pos, n, share in schedule(x.size // in_ch):
        chunk = np.ascontiguousarray(x[pos * in_ch:(pos + n) * in_ch])
        assert put(h, chunk.ctypes.data, n) == 0
        take(part(available(h), share))
    assert getattr(lib, f"nae_{prefix}_flush")(h) == 0
    assert put(h, x.ctypes.data, 1) == -5                              # NAE_ERR_STATE: put after flush
    take(available(h))
    assert available(h) == 0
    assert getattr(lib, f"nae_{prefix}_destroy")(h) == 0
    return np.concatenate(outs)


@pytest.mark.parametrize("rate,pitch,flags,lifter", [
    (1.0, 1.0, 0, False),                        # wire
    (1.5, f32(1 / 1.5), 0, False),               # vocoder only
    (f32(0.8), 1.0, 0, False),                   # transposer only
    (1.0, f32(2 ** (3 / 12)), 0, False),         # transposer, then vocoder
    (1.0, f32(2 ** (-4 / 12)), 0, False),        # vocoder, then transposer (planar mid FIFO)
    (1.0, f32(2 ** (-4 / 12)), 1, False),        # phase-locked
    (1.0, f32(2 ** (4 / 12)), 0, True),          # formant-preserving
])
def test_stretch_long_stream_equals_block(ctx, nae, rate, pitch, flags, lifter):
    ch, n_fft = 2, 1024
    x = (0.5 * orc.fill_uniform(L * ch, 23)).astype(np.float32)
    q = pv_ref.default_lifter(48000, n_fft) if lifter else 0
    h = C.c_void_p()
    assert ctx.lib.nae_stretch_create_formant(ctx.h, 48000, ch, rate, pitch, flags, n_fft, q, C.byref(h)) == 0
    y = drive(ctx.lib, h, "stretch", x, ch)
    want = block(ctx, nae, x, ch, rate, pitch, n_fft, lock=bool(flags), lifter=q)
    assert y.size == want.size
    assert same_bits(y, want)


@pytest.mark.parametrize("ch,rate,pitch", [(2, 1.0, 2 ** (3 / 12)), (2, 1.0, 2 ** (-4 / 12)), (1, 1.5, 1 / 1.5)])
def test_wsola_long_stream_equals_oracle(ctx, nae, ch, rate, pitch):
    x = orc.fill_uniform(L * ch, 29)
    h = C.c_void_p()
    assert ctx.lib.nae_wsola_create(ctx.h, 48000, ch, rate, pitch, C.byref(h)) == 0
    y = drive(ctx.lib, h, "wsola", x, ch)
    want = orc.st_process(x, ch, 48000, rate, pitch, chunk=PUTS)
    assert y.size == want.size
    assert same_bits(y, want)


@pytest.mark.parametrize("fmt_name,ch", [("FLT", 2), ("S16", 1)])
def test_swr_long_stream_equals_oracle(ctx, nae, fmt_name, ch):
    """44.1 -> 48 kHz; the references are built as tests/test_gpu_nodes.py builds them"""
    lib = ctx.lib
    if fmt_name == "FLT":
        m = orc.fill_uniform(L, 31)
        x = np.stack([m, -m], 1).reshape(-1).astype(np.float32)
        want_L, want_R = orc.swr_resample(m, 44100, 48000), orc.swr_resample(-m, 44100, 48000)
    else:
        x = (orc.fill_uniform(L, 31) * 30000).astype(np.int16)
        rc, f = orc.to_f32_interleaved(orc.FMT_S16, [x], L, 1)
        want_L = want_R = orc.swr_resample((f * np.float32(0.70710678118654752440)).astype(np.float32), 44100, 48000)
    h, got = C.c_void_p(), C.c_size_t()
    assert lib.nae_swr_create(ctx.h, getattr(nae, "FMT_" + fmt_name), 44100, ch, 48000, C.byref(h)) == 0
    outL, outR = [], []

    def convert(planes, n, max_out):
        bl, br = np.zeros(max(max_out, 1), np.float32), np.zeros(max(max_out, 1), np.float32)
        assert lib.nae_swr_convert_host(h, planes, n, bl.ctypes.data, br.ctypes.data, max_out, C.byref(got)) == 0
        outL.append(bl[: got.value]); outR.append(br[: got.value])
        return got.value

    for pos, n, share in schedule(L):
        chunk = np.ascontiguousarray(x[pos * ch:(pos + n) * ch])
        convert((C.c_void_p * 1)(chunk.ctypes.data), n, part(lib.nae_swr_buffered(h) + n, share))
    while convert(None, 0, 50000):
        pass
    assert lib.nae_swr_buffered(h) == 0
    assert lib.nae_swr_destroy(h) == 0
    assert same_bits(np.concatenate(outL), want_L)
    assert same_bits(np.concatenate(outR), want_R)


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (4096, 1000)])
def test_spectrum_long_stream_equals_block(ctx, nae, n_fft, hop):
    lib, ch, B = ctx.lib, 2, bins(n_fft)
    x = orc.fill_uniform(L * ch, 37)
    want = gpu_ex(ctx, nae, n_fft, hop, x, ch)[0]
    h, got = C.c_void_p(), C.c_size_t()
    assert lib.nae_spectrum_create(ctx.h, n_fft, hop, ch, C.byref(h)) == 0
    d_x, d_o = ctx.array(x), ctx.empty(want.size + ch * B)
    frames = 0
    for pos, n, share in schedule(L):
        assert lib.nae_spectrum_put(h, C.c_void_p(d_x.at(pos * ch)), n) == 0
        take = part(lib.nae_spectrum_available(h), share)
        assert lib.nae_spectrum_receive(h, C.c_void_p(d_o.at(frames * ch * B)), take, C.byref(got)) == 0
        assert got.value == take
        frames += take
    rest = lib.nae_spectrum_available(h)
    assert lib.nae_spectrum_receive(h, C.c_void_p(d_o.at(frames * ch * B)), rest, C.byref(got)) == 0
    frames += got.value
    assert lib.nae_spectrum_available(h) == 0
    assert lib.nae_spectrum_destroy(h) == 0
    assert frames == want.shape[0]
    out = d_o.download()[: want.size].reshape(want.shape)
    d_x.free(); d_o.free()
    assert same_bits(out, want)


def fir_case(n_fft, n_taps, ch, seed):
    """taps, 400 000 frames of noise, and the statement on the input extended by n_taps - 1 zero frames"""
    rng = np.random.default_rng(seed)
    taps = rng.uniform(-1, 1, n_taps).astype(np.float32)
    x = orc.fill_uniform(L * ch, seed)
    want = fir_ref.run(statement(fir_ref), taps, n_fft, np.concatenate([x, np.zeros((n_taps - 1) * ch, np.float32)]), ch=ch)
    return taps, x, want


@pytest.mark.parametrize("n_fft,n_taps,ch", [(512, 257, 2), (4096, 2049, 1), (1024, 2, 2)])
def test_fir_long_stream_equals_statement(ctx, nae, n_fft, n_taps, ch):
    """in_len + n_taps - 1 frames come out: the statement on the zero-extended input, and in its first in_len frames the block call"""
    taps, x, want = fir_case(n_fft, n_taps, ch, 43)
    h = C.c_void_p()
    assert ctx.lib.nae_fir_create(ctx.h, taps.ctypes.data, n_taps, n_fft, ch, C.byref(h)) == 0
    y = drive(ctx.lib, h, "fir", x, ch)
    assert y.size == (L + n_taps - 1) * ch
    assert same_bits(y, want)
    assert same_bits(y[: L * ch], gpu_fir(nae, ctx, taps, n_fft, x.reshape(1, L, ch)).reshape(-1))


def test_fir_long_stream_device_puts_and_receives(ctx, nae):
    """nae_fir_put / nae_fir_receive: the input FIFO is fed from device memory, and the output FIFO is popped device to device and then
    compacted in place on the same stream"""
    lib, n_fft, n_taps, ch = ctx.lib, 512, 257, 2
    taps, x, want = fir_case(n_fft, n_taps, ch, 47)
    h, got = C.c_void_p(), C.c_size_t()
    assert lib.nae_fir_create(ctx.h, taps.ctypes.data, n_taps, n_fft, ch, C.byref(h)) == 0
    d_x, d_o = ctx.array(x), ctx.empty(want.size + ch)
    frames = 0
    for pos, n, share in schedule(L):
        assert lib.nae_fir_put(h, C.c_void_p(d_x.at(pos * ch)), n) == 0
        take = part(lib.nae_fir_available(h), share)
        assert lib.nae_fir_receive(h, C.c_void_p(d_o.at(frames * ch)), take, C.byref(got)) == 0
        assert got.value == take
        frames += take
    assert lib.nae_fir_flush(h) == 0
    assert lib.nae_fir_put(h, C.c_void_p(d_x.ptr), 1) == -5                # NAE_ERR_STATE: put after flush
    rest = lib.nae_fir_available(h)
    assert lib.nae_fir_receive(h, C.c_void_p(d_o.at(frames * ch)), rest, C.byref(got)) == 0
    frames += got.value
    assert lib.nae_fir_available(h) == 0
    assert lib.nae_fir_destroy(h) == 0
    assert frames == L + n_taps - 1
    out = d_o.download()[: want.size]
    d_x.free(); d_o.free()
    assert same_bits(out, want)


# ---------------------------------------------------------------------------------------------------- the block-handle family
def loud_frames(seed, ch):
    """L frames of noise whose level wanders 14 dB under and over the -18 dB threshold: a signal the dynamics move, a key"""
    rng = np.random.default_rng(seed)
    t = np.arange(L)[:, None]
    return (rng.uniform(-1, 1, (L, ch)) * 10.0 ** ((-18.0 + 14.0 * np.sin(2 * np.pi * t / 411.0 + np.arange(ch))) / 20.0)).astype(np.float32)


def test_eq_long_stream_equals_statement(ctx, nae):
    """four sections; the statement's bits, which are the block call's"""
    coef, ch = eq_ref.cascade(4), 2
    x = orc.fill_uniform(L * ch, 53)
    y = drive(ctx.lib, nae.Eq(ctx, coef, ch).h, "eq", x, ch)
    want = eq_ref.run(statement(eq_ref), coef, x, ch=ch)
    assert y.size == L * ch and same_bits(y, want)
    assert same_bits(y, gpu_eq(nae, ctx, coef, x.reshape(1, L, ch)).reshape(-1))


def test_dyn_long_stream_equals_statement(ctx, nae):
    p, x = dyn_ref.params(lookahead=48, link=1, alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05)), loud_frames(59, 2)
    y = drive(ctx.lib, nae.Dyn(ctx, dyn_params(nae, p), 2).h, "dyn", x.reshape(-1), 2)
    want = dyn_ref.run(statement(dyn_ref), p, x)
    assert np.mean(want != x) > 0.5, "the statement's gain moves"
    assert y.size == want.size and same_bits(y, want.reshape(-1))


def test_dynkey_long_stream_equals_statement(ctx, nae):
    """a stereo key through four slow sections, interleaved into the puts: frames of 4 floats go in, frames of 2 come out"""
    dp = dyn_ref.params(lookahead=48, link=1, alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05))
    p = dynkey_ref.params(dp, 2, dynkey_ref.key_filters()[4])
    x, key = orc.fill_uniform(L * 2, 61).reshape(L, 2), loud_frames(67, 2)
    frames = np.ascontiguousarray(np.concatenate([x, key], 1)).reshape(-1)
    y = drive(ctx.lib, nae.DynKey(ctx, dynkey_params(nae, p), 2).h, "dynkey", frames, 2, in_ch=4)
    want = dynkey_ref.run(statement(dynkey_ref), p, x, key)
    assert np.mean(want != x) > 0.5, "the statement's gain moves"
    assert y.size == want.size and same_bits(y, want.reshape(-1))


def echo_case(seed):
    """delays 1500 and 1024 with cross and the designed pair of loop filters: the ring of 3072 samples wraps 130 times, and every put boundary
    falls somewhere else in it"""
    p = echo_ref.params((1500, 1024), -0.9, 1, 0.6, 0.8, echo_ref.loop_filters()[2])
    x = orc.fill_uniform(L * 2, seed).reshape(L, 2)
    want = echo_ref.run(statement(echo_ref), p, x)
    assert not np.array_equal(want[1500:], (0.8 * x[1500:].astype(np.float64)).astype(np.float32)), "the statement's repeats are there"
    return p, x, want


def test_echo_long_stream_equals_statement(ctx, nae):
    p, x, want = echo_case(71)
    y = drive(ctx.lib, nae.Echo(ctx, echo_params(nae, p), 2).h, "echo", x.reshape(-1), 2)
    assert y.size == want.size and same_bits(y, want.reshape(-1))


def test_echo_long_stream_device_puts_and_receives(ctx, nae):
    """nae_echo_put / nae_echo_receive: fed from device memory and popped device to device, as the FIR filter's handle above"""
    lib, ch = ctx.lib, 2
    p, x, want = echo_case(73)
    h, got = nae.Echo(ctx, echo_params(nae, p), ch).h, C.c_size_t()
    d_x, d_o = ctx.array(x.reshape(-1)), ctx.empty(want.size + ch)
    frames = 0
    for pos, n, share in schedule(L):
        assert lib.nae_echo_put(h, C.c_void_p(d_x.at(pos * ch)), n) == 0
        take = part(lib.nae_echo_available(h), share)
        assert lib.nae_echo_receive(h, C.c_void_p(d_o.at(frames * ch)), take, C.byref(got)) == 0
        assert got.value == take
        frames += take
    assert lib.nae_echo_flush(h) == 0
    assert lib.nae_echo_put(h, C.c_void_p(d_x.ptr), 1) == -5               # NAE_ERR_STATE: put after flush
    rest = lib.nae_echo_available(h)
    assert lib.nae_echo_receive(h, C.c_void_p(d_o.at(frames * ch)), rest, C.byref(got)) == 0
    frames += got.value
    assert lib.nae_echo_available(h) == 0
    assert lib.nae_echo_destroy(h) == 0
    assert frames == L
    out = d_o.download()[: want.size]
    d_x.free(); d_o.free()
    assert same_bits(out, want.reshape(-1))


def test_conv_long_stream_equals_statement(ctx, nae):
    """n_fft 512 with 2000 taps per channel (8 partitions): in_len + n_taps - 1 frames come out, the statement on the zero-extended input"""
    n_taps, ch = 2000, 2
    rng = np.random.default_rng(79)
    taps = (rng.uniform(-1, 1, (ch, n_taps)) * np.exp(-np.arange(n_taps) / 400.0)).astype(np.float32)
    x = orc.fill_uniform(L * ch, 79)
    y = drive(ctx.lib, nae.Conv(ctx, taps, ch, 512).h, "conv", x, ch)
    want = conv_ref.run(statement(conv_ref), taps, 512, np.concatenate([x, np.zeros((n_taps - 1) * ch, np.float32)]), ch=ch)
    assert y.size == (L + n_taps - 1) * ch and same_bits(y, want)


def test_denoise_long_stream_equals_statement(ctx, nae):
    """n_fft 1024 against a profile per channel; the level wanders around the profile's, so the gate opens and closes all along"""
    n_fft, ch = 1024, 2
    p = denoise_ref.params(n_fft, 2, 2, 1.0, 0.1)
    profile = denoise_ref.flat_profile(n_fft, ch, tilt_db=-3.0)
    x = denoise_ref.wander(np.random.default_rng(83), 1, L, ch, period=3.0 * n_fft)[0]
    d_p = ctx.array(profile.reshape(-1))
    h = nae.Denoise(ctx, denoise_params(nae, p), d_p.ptr, ch, ch).h
    ctx.sync()
    d_p.free()                                             # the handle has its own copy
    y = drive(ctx.lib, h, "denoise", x.reshape(-1), ch)
    want = denoise_ref.run(statement(denoise_ref), p, profile, x)
    assert 1e-3 < np.abs(want - x).max() and 1e-3 < np.abs(want - np.float32(0.1) * x).max(), "neither the input nor all at the floor gain"
    assert y.size == want.size and same_bits(y, want.reshape(-1))
