"""One contract for the put / receive handles (nae_fir, nae_conv, nae_eq, nae_dyn, nae_denoise, nae_dynkey, nae_echo, nae_mod, nae_stretch, nae_wsola),
through the C entries: puts that cross a unit boundary and leave a partial last unit, receives in pieces into device and host memory, the state
after the flush, and the output, bit for bit the block entry's on the whole input, in the length include/nae_gpu.h states.  For the FIR filter and
the convolution the block entry runs on the input extended by n_taps - 1 zero frames: that is what the header says a flushed handle delivers.
The WSOLA chain is the exception in what it is compared with: its output follows the put sequence (every put runs the stretcher on what has
arrived, and the flush counts from what was received), so `want` is not the block entry's output but the CPU oracle's for the same puts,
orc.st_process(..., chunk=the cuts), bit for bit and in length; there is no length the header could state and no look-ahead rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, STATE = 0, -1, -5                 # enum nae_status (include/nae_gpu.h)
CUTS = (1, 1023, 1025, 7)                      # then the rest: a unit boundary inside a put, single frames, a partial last unit
WSOLA_CUTS = (1, 1023, 5000, 7)                # the 5000-frame put crosses the stretcher's first sample_req
PIECE = 100                                    # max_frames of every receive


def spec_constant(name):
    """an integer constant of include/nae_dsp_spec.h (a product of 64 and another constant at most)"""
    text = open(os.path.join(ROOT, "include", "nae_dsp_spec.h")).read()
    value = re.search(r"#define\s+%s\s+(.+)" % name, text).group(1).strip()
    m = re.fullmatch(r"\(64 \* (\w+)\)", value)
    return 64 * spec_constant(m.group(1)) if m else int(value)


def noise(seed, n, ch):
    return np.random.default_rng(seed).uniform(-1, 1, (n, ch)).astype(np.float32)


def block(nae, ctx, x, out_len, call):
    """x[n, ch] -> [out_len, ch] through a block entry: call(src, in_len, ch, dst) returns its status"""
    n, ch = x.shape
    d_x, d_y = ctx.array(x.reshape(-1)), ctx.empty(out_len * ch)
    try:
        assert call(C.byref(nae.Sig.interleaved(d_x.ptr, n, ch)), n, ch, C.byref(nae.Sig.interleaved(d_y.ptr, out_len, ch))) == OK
        return d_y.download().reshape(out_len, ch)
    finally:
        d_x.free()
        d_y.free()


def zero_tail(x, frames):
    return np.concatenate([x, np.zeros((frames, x.shape[1]), np.float32)])


# every case: (x[n, ch], create(handle pointer) -> status, the block entry's output on the whole input, look-ahead or None)
def fir_case(nae, ctx):
    lib, x = ctx.lib, noise(1, 3000, 2)
    taps = nae.Context.fir_design("lowpass", 48000, 0.0, 3000.0, 31)
    ext = zero_tail(x, 30)
    want = block(nae, ctx, ext, len(ext), lambda s, n, ch, d: lib.nae_fir_block_f32(ctx.h, taps.ctypes.data, 31, 512, s, n, ch, 1, d))
    return x, lambda h: lib.nae_fir_create(ctx.h, taps.ctypes.data, 31, 512, 2, h), want, None


def conv_case(nae, ctx):
    lib, x = ctx.lib, noise(2, 3000, 2)
    taps = (noise(3, 700, 2).T * np.exp(-np.arange(700) / 150.0)).astype(np.float32)      # [2][700]: one response per channel
    taps = np.ascontiguousarray(taps)
    ext = zero_tail(x, 699)
    want = block(nae, ctx, ext, len(ext), lambda s, n, ch, d: lib.nae_conv_block_f32(ctx.h, taps.ctypes.data, 700, 2, 512, s, n, ch, 1, d))
    return x, lambda h: lib.nae_conv_create(ctx.h, taps.ctypes.data, 700, 2, 512, 2, h), want, None


def eq_case(nae, ctx):
    lib, x = ctx.lib, noise(4, 2500, 2)
    coef = np.ascontiguousarray([nae.Context.eq_design("peak", 48000, 1000.0, 6.0, 1.0), nae.Context.eq_design("highshelf", 48000, 6000.0, -4.0)])
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_eq_block_f32(ctx.h, coef.ctypes.data, 2, s, n, ch, 1, d))
    return x, lambda h: lib.nae_eq_create(ctx.h, coef.ctypes.data, 2, 2, h), want, None


def dyn_case(nae, ctx):
    lib, x = ctx.lib, noise(5, 2500, 2)
    params = nae.Context.dyn_design(48000, lookahead_s=0.001, link=True)
    assert params.lookahead == 48 and params.link == 1
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_dyn_block_f32(ctx.h, C.byref(params), s, n, ch, 1, d))
    return x, lambda h: lib.nae_dyn_create(ctx.h, C.byref(params), 2, h), want, 48


def denoise_case(nae, ctx):
    """n_fft 512 against the profile nae_denoise_profile_f32 measures on device from an excerpt of steady noise; the input's level wanders
    around the excerpt's, so the gate opens and closes.  The handle copies the profile at creation"""
    lib = ctx.lib
    t = np.arange(3000)[:, None]
    x = (noise(7, 3000, 2) * 10.0 ** (14.0 * np.sin(2 * np.pi * t / 1500.0 + np.array([0.0, 2.0])) / 20.0)).astype(np.float32)
    params = nae.DenoiseParams(512, 2, 2, 1.0, 0.25)
    d_n, d_p = ctx.array(noise(8, 4096, 2).reshape(-1)), ctx.empty(2 * 257)
    assert lib.nae_denoise_profile_f32(ctx.h, 512, C.byref(nae.Sig(d_n.ptr, 0, 1, 2)), 4096, 2, d_p.ptr) == OK
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_denoise_block_f32(ctx.h, C.byref(params), d_p.ptr, 2, s, n, ch, 1, d))
    assert 1e-3 < np.abs(want - x).max() and 1e-3 < np.abs(want - np.float32(0.25) * x).max(), "neither the input nor all at the floor gain"
    d_n.free()
    return x, lambda h: lib.nae_denoise_create(ctx.h, C.byref(params), d_p.ptr, 2, 2, h), want, None


def dynkey_case(nae, ctx):
    """self-keyed through two sections (key_ch = 0), so a put frame is `ch` floats; look-ahead 48"""
    lib, x = ctx.lib, noise(9, 2500, 2)
    coef = [nae.Context.eq_design("highpass", 48000, 150.0), nae.Context.eq_design("peak", 48000, 3000.0, 6.0, 1.0)]
    params = nae.DynKeyParams.make(nae.Context.dyn_design(48000, lookahead_s=0.001, link=True), 0, coef)
    assert params.dyn.lookahead == 48 and params.n_sections == 2
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_dynkey_block_f32(ctx.h, C.byref(params), s, None, n, ch, 1, d))
    return x, lambda h: lib.nae_dynkey_create(ctx.h, C.byref(params), 2, h), want, 48


def echo_case(nae, ctx):
    """ping-pong at delays 1024 and 1500 through two sections; 3 R + 7 frames wrap the handle's ring three times"""
    lib = ctx.lib
    coef = [nae.Context.eq_design("lowpass", 48000, 4000.0), nae.Context.eq_design("highpass", 48000, 150.0)]
    params = nae.EchoParams.make((1024, 1500), -0.9, True, 0.6, 0.8, coef)
    x = noise(10, 3 * 3072 + 7, 2)
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_echo_block_f32(ctx.h, C.byref(params), s, n, ch, 1, d))
    return x, lambda h: lib.nae_echo_create(ctx.h, C.byref(params), 2, h), want, None


def mod_case(nae, ctx):
    """a flanger with feedback and two voices (runs of 16 samples); 3 * 4096 + 7 frames wrap the handle's ring three times"""
    lib = ctx.lib
    params = nae.ModParams.make(24.0, 7.0, 0.9, 0.6, 0.8, (1 << 32) // 997, 3, 1 << 30, (0, 1 << 31))
    x = noise(11, 3 * 4096 + 7, 2)
    want = block(nae, ctx, x, len(x), lambda s, n, ch, d: lib.nae_mod_block_f32(ctx.h, C.byref(params), s, n, ch, 1, d))
    return x, lambda h: lib.nae_mod_create(ctx.h, C.byref(params), 2, h), want, None


def stretch_case(nae, ctx):
    lib, x = ctx.lib, noise(6, 8192, 1)
    pitch = float(np.float32(2 ** (3 / 12)))   # the handle takes floats
    out_len = nae.Context.stretch_plan(1.0, pitch, len(x)).out_len
    want = block(nae, ctx, x, out_len, lambda s, n, ch, d: lib.nae_stretch_block_f32(ctx.h, 1.0, pitch, s, n, ch, 1, d))
    return x, lambda h: lib.nae_stretch_create(ctx.h, 48000, 1, 1.0, pitch, h), want, None


def wsola_case(order, rate, pitch):
    """48 kHz stereo, one case per stage order (0: stretcher, filter, transposer; 1: filter, transposer, stretcher; 2: transposer, filter,
    stretcher)"""
    def case(nae, ctx):
        n = 20000
        assert ctx.wsola_plan(48000, 2, rate, pitch, n).order == order
        x = orc.fill_uniform(n * 2, 40 + order)
        want = orc.st_process(x, 2, 48000, rate, pitch, chunk=list(WSOLA_CUTS) + [n - sum(WSOLA_CUTS)]).reshape(-1, 2)
        return x.reshape(n, 2), lambda h: ctx.lib.nae_wsola_create(ctx.h, 48000, 2, rate, pitch, h), want, None
    return case


CASES = {"fir": fir_case, "conv": conv_case, "eq": eq_case, "dyn": dyn_case, "denoise": denoise_case, "dynkey": dynkey_case, "echo": echo_case,
         "mod": mod_case, "stretch": stretch_case,
         "wsola0": wsola_case(0, 1.0, 2 ** (3 / 12)), "wsola1": wsola_case(1, 1.5, 1 / 1.5), "wsola2": wsola_case(2, 0.8, 1.0)}
# the lengths the header states: in_len + n_taps - 1, in_len, the plan's out_len (stretch_case: `want` has it)
OUT_LEN = {"fir": 3000 + 31 - 1, "conv": 3000 + 700 - 1, "eq": 2500, "dyn": 2500, "denoise": 3000, "dynkey": 2500, "echo": 3 * 3072 + 7,
           "mod": 3 * 4096 + 7}


@pytest.mark.parametrize("prefix", CASES)
def test_handle_contract(nae, ctx, prefix):
    lib = ctx.lib
    x, create, want, lookahead = CASES[prefix](nae, ctx)
    n, ch = x.shape
    if prefix in OUT_LEN:
        assert len(want) == OUT_LEN[prefix]
    family, cuts = (prefix[:-1], WSOLA_CUTS) if prefix.startswith("wsola") else (prefix, CUTS)
    entry = {name: getattr(lib, f"nae_{family}_{name}") for name in ("put", "put_host", "flush", "available", "receive", "receive_host", "destroy")}
    h = C.c_void_p()
    assert create(C.byref(h)) == OK
    d_x, d_piece = ctx.array(x.reshape(-1)), ctx.empty(PIECE * ch)
    got, parts, puts, takes = C.c_size_t(), [], 0, 0

    def put(pos, k):
        nonlocal puts
        puts += 1
        if puts % 2:
            return entry["put"](h, d_x.at(pos * ch), k)
        return entry["put_host"](h, np.ascontiguousarray(x[pos:pos + k]).ctypes.data, k)

    def drain():
        """everything available, in pieces of at most PIECE frames, into device and host memory in turn"""
        nonlocal takes
        received = 0
        while True:
            before = entry["available"](h)
            got.value = 77
            assert entry["receive"](h, d_piece.ptr, 0, C.byref(got)) == OK and got.value == 0, "max_frames = 0"
            assert entry["available"](h) == before
            if before == 0:
                return received
            takes += 1
            if takes % 2:
                assert entry["receive"](h, d_piece.ptr, PIECE, C.byref(got)) == OK
                piece = d_piece.download()
            else:
                piece = np.empty(PIECE * ch, np.float32)
                assert entry["receive_host"](h, piece.ctypes.data, PIECE, C.byref(got)) == OK
            assert got.value == min(before, PIECE)
            assert entry["available"](h) == before - got.value, "available falls by exactly what was received"
            parts.append(piece[:got.value * ch].copy())
            received += got.value

    try:
        pos, received = 0, 0
        for k in cuts + (n - sum(cuts),):
            assert put(pos, k) == OK
            pos += k
            if lookahead is not None:
                chunk = spec_constant("NAE_DYN_CHUNK")
                assert entry["available"](h) + received == max(pos - lookahead, 0) // chunk * chunk, "whole chunks whose look-ahead is complete"
            received += drain()
        assert pos == n
        assert entry["flush"](h) == OK
        released = entry["available"](h)
        assert received + released == len(want), "the length the header states"
        assert entry["flush"](h) == OK and entry["available"](h) == released, "a second flush releases nothing more"
        for k in (1, 0):
            assert entry["put"](h, d_x.ptr, k) == STATE and entry["put_host"](h, x.ctypes.data, k) == STATE, "put after flush"
        assert entry["available"](h) == released
        received += drain()
        assert entry["available"](h) == 0
    finally:
        assert entry["destroy"](h) == OK
        d_x.free()
        d_piece.free()
    out = np.concatenate(parts).reshape(-1, ch)
    assert out.shape == want.shape
    assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), int(np.count_nonzero(out != want))
