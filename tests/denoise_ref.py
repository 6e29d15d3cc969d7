"""ctypes binding of the CPU statement of the spectral gate (tests/denoise_ref/ref_denoise.c), built by tests/cstatement.py, its float64
numpy restatement, and the signals and parameter sets the tests share."""
import ctypes as C
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "denoise_ref", "ref_denoise.c")
SIZES = (512, 1024, 2048, 4096)
MAX_TIME, MAX_FREQ = 8, 4          # NAE_DENOISE_MAX_TIME, NAE_DENOISE_MAX_FREQ
OLA_GAIN = 2.0 / 3.0               # NAE_OLA_GAIN


class Params(C.Structure):
    """nae_denoise_params of include/nae_gpu.h"""
    _fields_ = [("n_fft", C.c_int), ("time_smooth", C.c_int), ("freq_smooth", C.c_int), ("thr_scale", C.c_float), ("floor_gain", C.c_float)]


def params(n_fft=512, time_smooth=2, freq_smooth=2, thr_scale=4.0, floor_gain=0.25):
    return Params(n_fft, time_smooth, freq_smooth, thr_scale, floor_gain)


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in Params._fields_)


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_denoise_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_denoise_profile.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.ref_denoise_design.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    return L


def frames_of(n_fft, n):
    """frames 0 ... B + 2 of a signal of n samples"""
    h = n_fft // 4
    return (n + h - 1) // h + 3


def run(L, p, profile, x, detail=False, mask=None):
    """x[n, ch] f32 and profile[1 or ch, n_fft / 2 + 1] -> y[n, ch]; detail: also the decisions d[ch, frames, bins] (uint8) and the counts
    c[ch, frames, bins]; mask: decisions [ch, frames, bins] to use in place of the statement's own"""
    x = np.ascontiguousarray(x, np.float32)
    profile = np.ascontiguousarray(profile, np.float32).reshape(-1, p.n_fft // 2 + 1)
    n, ch = x.shape
    y = np.zeros_like(x)
    F, K = frames_of(p.n_fft, n), p.n_fft // 2 + 1
    d = np.zeros((ch, F, K), np.uint8)
    c = np.zeros((ch, F, K), np.int32)
    for k in range(ch):
        prof = np.ascontiguousarray(profile[k if profile.shape[0] > 1 else 0])
        m = np.ascontiguousarray(mask[k], np.uint8) if mask is not None else None
        rc = L.ref_denoise_run(p.n_fft, p.time_smooth, p.freq_smooth, p.thr_scale, p.floor_gain, prof.ctypes.data, x.ctypes.data + 4 * k, n, ch,
                               y.ctypes.data + 4 * k, d[k].ctypes.data, c[k].ctypes.data, m.ctypes.data if m is not None else None)
        assert rc == 0
    return (y, d, c) if detail else y


def run_streams(L, p, profile, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, profile, s) for s in x])


def profile(L, n_fft, x):
    """x[len, ch] -> the noise profile [ch, n_fft / 2 + 1], or None where the excerpt holds no whole frame"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    out = np.zeros((ch, n_fft // 2 + 1), np.float32)
    for k in range(ch):
        if L.ref_denoise_profile(n_fft, x.ctypes.data + 4 * k, n, ch, out[k].ctypes.data) != 0:
            return None
    return out


def design(L, reduction_db, sensitivity_db):
    thr, floor = C.c_float(), C.c_float()
    L.ref_denoise_design(reduction_db, sensitivity_db, C.byref(thr), C.byref(floor))
    return thr.value, floor.value


# ---------------------------------------------------------------------------------------------------- the float64 restatement
def hann64(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames64(n_fft, x):
    """x[n] -> the windowed frames [B + 3, n_fft] in float64: frame f starts at (f - 3) H, zero outside the signal"""
    h, n = n_fft // 4, len(x)
    F = frames_of(n_fft, n)
    pad = np.zeros(3 * h + (F + 1) * h, np.float64)
    pad[3 * h:3 * h + n] = x
    idx = np.arange(F)[:, None] * h + np.arange(n_fft)[None, :]
    return pad[idx] * hann64(n_fft)[None, :]


def power64(n_fft, x):
    """the power of every frame and bin, and the spectra"""
    X = np.fft.rfft(frames64(n_fft, np.asarray(x, np.float64)), axis=1)
    return X.real ** 2 + X.imag ** 2, X


def counts64(d, tn, fn):
    """decisions d[frames, bins] -> the smoothed counts c, in integers"""
    F, K = d.shape
    M = K - 1
    d = d.astype(np.int64)
    v = np.zeros_like(d)
    for j in range(-tn, tn + 1):
        lo, hi = max(0, -j), min(F, F - j)
        v[lo:hi] += (tn + 1 - abs(j)) * d[lo + j:hi + j]
    c = np.zeros_like(d)
    k = np.arange(K)
    for i in range(-fn, fn + 1):
        kk = np.abs(k + i)
        kk = np.where(kk > M, 2 * M - kk, kk)
        c += (fn + 1 - abs(i)) * v[:, kk]
    return c


def run64(p, prof, x, mask=None):
    """one channel x[n] against prof[bins] in float64 numpy -> (y[n], the ratio p / threshold [frames, bins], the decisions); mask: decisions to use"""
    n_fft, h, n = p.n_fft, p.n_fft // 4, len(x)
    pw, X = power64(n_fft, x)
    thr = np.asarray(prof, np.float64)[None, :] * float(p.thr_scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = pw / thr
    d = (pw > thr) if mask is None else np.asarray(mask, bool)
    c = counts64(d, p.time_smooth, p.freq_smooth)
    C_full = (p.time_smooth + 1) ** 2 * (p.freq_smooth + 1) ** 2
    g = np.where(c == C_full, 1.0, float(p.floor_gain) + (1.0 - float(p.floor_gain)) * (c / C_full))
    yf = np.fft.irfft(g * X, n=n_fft, axis=1) * hann64(n_fft)[None, :]
    F = yf.shape[0]
    out = np.zeros((F + 3) * h, np.float64)
    for f in range(F):
        out[f * h:f * h + n_fft] += yf[f]
    return out[3 * h:3 * h + n] * OLA_GAIN, ratio, d


# ---------------------------------------------------------------------------------------------------- signals
def wander(rng, n_streams, n, ch, level=1.0, depth_db=14.0, period=1500.0, shared=False):
    """noise whose level wanders far under and far over `level`, another phase per stream and channel (tests/test_gpu_dyn.py's `loud`)"""
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * level * 10.0 ** (depth_db * np.sin(2 * np.pi * t / period + ph) / 20.0)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def flat_profile(n_fft, ch=1, level=1.0, tilt_db=0.0):
    """the expected power of Hann-windowed uniform noise of amplitude `level` (variance level^2 / 3, sum of hann^2 = 3 N / 8), flat or tilted by
    tilt_db from bin 0 to bin N / 2, each channel 1 dB above the one before"""
    k = np.arange(n_fft // 2 + 1) / (n_fft // 2)
    base = level * level / 3.0 * 0.375 * n_fft * 10.0 ** (tilt_db * k / 10.0)
    return np.stack([base * 10.0 ** (0.1 * c) for c in range(ch)]).astype(np.float32)


def open_share(d):
    return float(np.mean(d))
