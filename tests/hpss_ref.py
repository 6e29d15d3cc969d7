"""ctypes binding of the CPU statement of the harmonic/percussive separation (tests/hpss_ref/ref_hpss.c), built by tests/cstatement.py, its
float64 numpy restatement, and the signals and parameter sets the tests share."""
import ctypes as C
import os

import numpy as np

import cstatement
from denoise_ref import OLA_GAIN, frames_of, hann64, power64, wander  # noqa: F401 — the STFT geometry and the noise are K13's

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hpss_ref", "ref_hpss.c")
SIZES = (512, 1024, 2048, 4096)
MAX_SPAN = 8                       # NAE_HPSS_MAX_SPAN
MIN_DB, MAX_DB = -120.0, 12.0      # NAE_HPSS_MIN_DB, NAE_HPSS_MAX_DB
MASKS = ("soft", "hard")           # `hard` of nae_hpss_params: 0, 1


class Params(C.Structure):
    """nae_hpss_params of include/nae_gpu.h"""
    _fields_ = [("n_fft", C.c_int), ("time_span", C.c_int), ("freq_span", C.c_int), ("hard", C.c_int), ("gain_h", C.c_float), ("gain_p", C.c_float)]


def params(n_fft=512, time_span=8, freq_span=8, hard=0, gain_h=1.0, gain_p=0.0):
    return Params(n_fft, time_span, freq_span, hard, gain_h, gain_p)


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in Params._fields_)


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_hpss_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_hpss_gain.argtypes = [C.c_double]
    L.ref_hpss_gain.restype = C.c_float
    return L


def run(L, p, x, detail=False):
    """x[n, ch] f32 -> y[n, ch]; detail: also the keys q, the medians hq and pq (uint16) and the mask m (f32), each [ch, frames, bins]"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    y = np.zeros_like(x)
    F, K = frames_of(p.n_fft, n), p.n_fft // 2 + 1
    q, hq, pq = (np.zeros((ch, F, K), np.uint16) for _ in range(3))
    m = np.zeros((ch, F, K), np.float32)
    for k in range(ch):
        rc = L.ref_hpss_run(p.n_fft, p.time_span, p.freq_span, p.hard, p.gain_h, p.gain_p, x.ctypes.data + 4 * k, n, ch, y.ctypes.data + 4 * k,
                            *((a[k].ctypes.data for a in (q, hq, pq, m)) if detail else (None,) * 4))
        assert rc == 0
    return (y, q, hq, pq, m) if detail else y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


# ---------------------------------------------------------------------------------------------------- keys
def value(q):
    """the float whose bits are q << 16"""
    return (np.asarray(q, np.uint32) << 16).view(np.float32)


def key64(pw):
    """the key of a float64 power: the largest q with value(q) <= pw"""
    f = np.asarray(pw, np.float64).astype(np.float32)
    f = np.where(f.astype(np.float64) > pw, np.nextafter(f, np.float32(0)), f).astype(np.float32)
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def near_boundary(pw, rel=1e-5):
    """where a float64 power lies within rel of one of the two key boundaries around it (an exact zero lies on none)"""
    q = key64(pw).astype(np.uint32)
    lo, hi = value(q).astype(np.float64), value(q + 1).astype(np.float64)
    return (pw > 0) & ((pw - lo <= rel * pw) | (hi - pw <= rel * pw))


def mir(k, M):
    k = np.abs(k)
    return np.where(k > M, 2 * M - k, k)


def windows(a, tn, fn):
    """a[frames, bins] -> (the 2 tn + 1 values over time [frames, bins, 2 tn + 1], zero outside the frames; the 2 fn + 1 values over the
    mirrored bins [frames, bins, 2 fn + 1])"""
    F, K = a.shape
    pad = np.zeros((F + 2 * tn, K), a.dtype)
    pad[tn:tn + F] = a
    over_t = np.stack([pad[j:j + F] for j in range(2 * tn + 1)], axis=2)
    k = np.arange(K)
    over_f = np.stack([a[:, mir(k + i, K - 1)] for i in range(-fn, fn + 1)], axis=2)
    return over_t, over_f


def medians_by_sort(q, tn, fn):
    """keys q[frames, bins] -> (Hq, Pq) by a brute-force sort: the element of rank (count - 1) / 2"""
    over_t, over_f = windows(q, tn, fn)
    return np.sort(over_t, axis=2)[:, :, tn], np.sort(over_f, axis=2)[:, :, fn]


def mask_of(hq, pq, hard):
    """the mask of the medians' keys, in float64 (the soft one before its rounding to f32)"""
    if hard:
        return (hq >= pq).astype(np.float64)
    h, p = value(hq).astype(np.float64), value(pq).astype(np.float64)
    s = h + p
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s == 0, 0.5, h / s)


# ---------------------------------------------------------------------------------------------------- the float64 restatement
def run64(p, x, mask=None):
    """one channel x[n] in float64 numpy -> (y[n], the powers [frames, bins], the keys of the powers, Hq, Pq); np.median over the float64
    powers, then the key of the result.  mask: a mask [frames, bins] to use in place of the restatement's own"""
    n_fft, h, n = p.n_fft, p.n_fft // 4, len(x)
    pw, X = power64(n_fft, x)
    over_t, over_f = windows(pw, p.time_span, p.freq_span)
    hq, pq = key64(np.median(over_t, axis=2)), key64(np.median(over_f, axis=2))
    m = mask_of(hq, pq, p.hard) if mask is None else np.asarray(mask, np.float64)
    g = float(p.gain_p) + (float(p.gain_h) - float(p.gain_p)) * m
    yf = np.fft.irfft(g * X, n=n_fft, axis=1) * hann64(n_fft)[None, :]
    F = yf.shape[0]
    out = np.zeros((F + 3) * h, np.float64)
    for f in range(F):
        out[f * h:f * h + n_fft] += yf[f]
    return out[3 * h:3 * h + n] * OLA_GAIN, pw, key64(pw), hq, pq


def design64(db):
    """one level of nae_hpss_design in float64 -> f32"""
    return np.float32(0.0) if db <= MIN_DB else np.float32(10.0 ** (db / 20.0))


# ---------------------------------------------------------------------------------------------------- signals
def bursts(rng, n, ch, n_fft, on=2, period=12):
    """K13's noise with a wandering level in bursts of `on` hop blocks every `period`, digital silence between them: most frames see nothing
    but zeros and their keys are exactly 0 in f32 as in float64"""
    h = n_fft // 4
    x = wander(rng, 1, n, ch, period=3.0 * n_fft)[0]
    gate = ((np.arange(n) // h) % period) < on
    return (x * gate[:, None]).astype(np.float32)


def chord_and_clicks(n, rate=48000.0):
    """a steady two-tone chord (440 Hz and 660 Hz, 0.25 each) -> tone[n], and a click train (one sample of 0.9 every 4800 samples, alternating
    sign) -> clicks[n], both f32; their sum is the separation's test signal"""
    t = np.arange(n) / rate
    tone = 0.25 * np.sin(2 * np.pi * 440.0 * t) + 0.25 * np.sin(2 * np.pi * 660.0 * t + 1.0)
    clicks = np.zeros(n)
    at = np.arange(2400, n, 4800)
    clicks[at] = 0.9 * (-1.0) ** np.arange(len(at))
    return tone.astype(np.float32), clicks.astype(np.float32)
