"""ctypes binding of the CPU statement of the modulated delay (tests/mod_ref/ref_mod.c), built by tests/cstatement.py, a float64 numpy
restatement of it and of the design, and the parameter sets the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mod_ref", "ref_mod.c")
CHUNK = 1024                                                        # NAE_EQ_CHUNK: the handle's unit
MIN_DELAY, MAX_DELAY, MAX_VOICES, MAX_FEEDBACK = 2.0, 3070.0, 4, 0.95   # NAE_MOD_* of include/nae_dsp_spec.h
SINE, TRIANGLE = 0, 1
M32 = 0xffffffff


class Params(C.Structure):
    """nae_mod_params of include/nae_gpu.h"""
    _fields_ = [("delay", C.c_double), ("depth", C.c_double), ("feedback", C.c_double), ("wet", C.c_double), ("dry", C.c_double),
                ("rate_inc", C.c_uint32), ("phase0", C.c_uint32), ("phase_ch", C.c_uint32), ("n_voices", C.c_int),
                ("voice_phase", C.c_uint32 * MAX_VOICES), ("shape", C.c_int)]


def half_up(v):
    """llround of a value that is not negative: halves away from zero"""
    return int(v) + (1 if v - int(v) >= 0.5 else 0)


def hz(rate_hz, sample_rate=48000):
    """rate_inc of a rate in hertz, as the design makes it"""
    return half_up((rate_hz / float(sample_rate)) * 4294967296.0) & M32


def spread_voices(n):
    """the design's voice phases: n voices evenly over a turn"""
    return tuple(((v << 32) // n) & M32 for v in range(n))


def params(delay, depth, feedback=0.0, wet=1.0, dry=1.0, rate_inc=hz(0.8), phase0=0, phase_ch=0, voice_phase=(0,), shape=SINE, n_voices=None):
    """voice_phase: one offset per voice; n_voices: a count that differs from len(voice_phase), for the rejections"""
    p = Params()
    p.delay, p.depth, p.feedback, p.wet, p.dry = delay, depth, feedback, wet, dry
    p.rate_inc, p.phase0, p.phase_ch, p.shape = rate_inc & M32, phase0 & M32, phase_ch & M32, shape
    p.n_voices = len(voice_phase) if n_voices is None else n_voices
    for v, ph in enumerate(voice_phase[:MAX_VOICES]):
        p.voice_phase[v] = ph & M32
    return p


def as_tuple(p):
    """the record's fields, for comparing two records"""
    return (p.delay, p.depth, p.feedback, p.wet, p.dry, p.rate_inc, p.phase0, p.phase_ch, p.n_voices, tuple(p.voice_phase), p.shape)


def sub_block(p):
    """L, the samples the GPU computes in parallel: 64 without feedback, else min(64, floor(delay - depth) - 1) ("K17 modulated delay")"""
    return 64 if p.feedback == 0.0 else min(64, math.floor(p.delay - p.depth) - 1)


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_mod_check.argtypes = [C.POINTER(Params), C.c_int]
    L.ref_mod_design.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(Params)]
    L.ref_mod_lfo.argtypes = [C.c_int, C.c_uint32]
    L.ref_mod_lfo.restype = C.c_double
    L.ref_mod_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    return L


def run(L, p, x, want_line=False):
    """x[n, ch] f32 -> y[n, ch] f32 (and the line w[n, ch]): the statement"""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[1] in (1, 2)
    y, line = np.zeros_like(x), np.zeros_like(x)
    rc = L.ref_mod_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, line.ctypes.data if want_line else None)
    assert rc == 0, rc
    return (y, line) if want_line else y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def lfo_np(shape, phi):
    """the LFO at the phases phi (uint32 array), every step one float64 operation"""
    t = phi.astype(np.uint32).view(np.int32).astype(np.float64) * 2.0 ** -31
    if shape == SINE:
        y = (4.0 * t) * (1.0 - np.abs(t))
        return (0.225 * ((y * np.abs(y)) - y)) + y
    return (2.0 * np.abs(t)) - 1.0


def _taps(p, n, c):
    """per voice: k (int64) and the four coefficients at the sample indices n (uint64 array) of channel c"""
    out = []
    for v in range(p.n_voices):
        base = (p.phase0 + p.voice_phase[v] + (p.phase_ch if c == 1 else 0)) & M32
        phi = ((n * np.uint64(p.rate_inc) + np.uint64(base)) & np.uint64(M32)).astype(np.uint32)
        d = np.float64(p.delay) + (np.float64(p.depth) * lfo_np(p.shape, phi))
        kf = np.floor(d)
        f = d - kf
        fm1, fm2, fp1 = f - 1.0, f - 2.0, f + 1.0
        ca = ((-(f * fm1)) * fm2) * (1.0 / 6.0)
        cb = ((fp1 * fm1) * fm2) * 0.5
        cc = ((-(fp1 * f)) * fm2) * 0.5
        ce = ((fp1 * f) * fm1) * (1.0 / 6.0)
        out.append((kf.astype(np.int64), ca, cb, cc, ce))
    return out


def run_np(p, x):
    """float64 numpy restatement: every step one float64 operation in the specification's order, the line np.float32.  Without feedback the
    line is the input and every sample is computed at once; with it, a loop over the samples"""
    x = np.ascontiguousarray(x, np.float32)
    n_len, ch = x.shape
    f64, f32 = np.float64, np.float32
    g, wet, dry, inv = f64(p.feedback), f64(p.wet), f64(p.dry), f64(1.0) / f64(p.n_voices)
    y = np.zeros((n_len, ch), f32)
    idx = np.arange(n_len, dtype=np.int64)
    for c in range(ch):
        taps = _taps(p, idx.astype(np.uint64), c)
        xd = x[:, c].astype(f64)
        if g == 0.0:
            pad = np.concatenate([np.zeros(4096, f64), xd])        # pad[4096 + i] = w[i]; an index below 0 reads 0
            v = None
            for k, ca, cb, cc, ce in taps:
                at = idx - k + 4096
                tap = (((ca * pad[at + 1]) + (cb * pad[at])) + (cc * pad[at - 1])) + (ce * pad[at - 2])
                v = tap if v is None else v + tap
            y[:, c] = ((dry * xd) + (wet * (v * inv))).astype(f32)
            continue
        w = np.zeros(4096 + n_len, f32)                             # w[4096 + i]
        for i in range(n_len):
            v = None
            for k, ca, cb, cc, ce in taps:
                at = i - int(k[i]) + 4096
                tap = (((ca[i] * f64(w[at + 1])) + (cb[i] * f64(w[at]))) + (cc[i] * f64(w[at - 1]))) + (ce[i] * f64(w[at - 2]))
                v = tap if v is None else v + tap
            u = v * inv
            w[4096 + i] = f32(xd[i] + (g * u))
            y[i, c] = f32((dry * xd[i]) + (wet * u))
    return y


def design(sample_rate, rate_hz=0.8, delay_ms=12.0, depth_ms=3.0, feedback=0.0, voices=3, spread=0.5, shape=SINE, wet=0.5, dry=1.0):
    """float64 restatement of nae_mod_design (include/nae_gpu.h); None where the library answers NAE_ERR_INVALID"""
    args = (rate_hz, delay_ms, depth_ms, feedback, spread, wet, dry)
    if sample_rate <= 0 or not all(math.isfinite(a) for a in args):
        return None
    if not 0.0 <= rate_hz <= 20.0 or depth_ms < 0.0 or not abs(feedback) <= MAX_FEEDBACK or not 0.0 <= spread <= 1.0:
        return None
    if not 1 <= voices <= MAX_VOICES or shape not in (SINE, TRIANGLE):
        return None
    delay = float((np.float64(delay_ms) * np.float64(1e-3)) * np.float64(sample_rate))
    depth = float((np.float64(depth_ms) * np.float64(1e-3)) * np.float64(sample_rate))
    if not delay - depth >= MIN_DELAY or not delay + depth <= MAX_DELAY:
        return None
    return params(delay, depth, feedback, wet, dry, half_up((rate_hz / float(sample_rate)) * 4294967296.0) & M32, 0,
                  half_up(spread * 2147483648.0), spread_voices(voices), shape)
