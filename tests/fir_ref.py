"""ctypes binding of the CPU statement of the FIR filter (tests/fir_ref/ref_fir.c), built by tests/cstatement.py, and the float64 restatements
the CPU tests compare against: the direct convolution and the Kaiser-8 designs."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fir_ref", "ref_fir.c")
SIZES = (512, 1024, 2048, 4096)
KINDS = ("lowpass", "highpass", "bandpass", "bandstop")
KAISER_BETA = 8.0


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_fir_pick_n_fft.argtypes = [C.c_int]
    L.ref_fir_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    return L


def pick_n_fft(n_taps):
    """DESIGN.md §3, "K9 FIR filter": the smallest supported N with N / 2 + 1 >= n_taps, else 0"""
    if n_taps < 1:
        return 0
    return next((n for n in SIZES if n // 2 + 1 >= n_taps), 0)


def run(L, taps, n_fft, x, ch=1):
    """x: interleaved [n * ch] f32 -> interleaved [n * ch], every channel filtered by `taps` at frame size n_fft"""
    taps = np.ascontiguousarray(taps, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    n = x.size // ch
    for c in range(ch):
        rc = L.ref_fir_run(taps.ctypes.data, taps.size, n_fft, x.ctypes.data + 4 * c, n, ch, y.ctypes.data + 4 * c)
        assert rc == 0, rc
    return y


def direct(taps, x):
    """float64 causal convolution y[n] = sum_j h[j] x[n - j], n < len(x)"""
    return np.convolve(np.asarray(x, np.float64), np.asarray(taps, np.float64))[: len(x)]


def _i0(x):
    """the power series of I0 the library's tables use (the transposer's), in double"""
    s = term = 1.0
    q = x * x / 4.0
    for k in range(1, 64):
        term *= q / (float(k) * float(k))
        s += term
        if term < 1e-18 * s:
            break
    return s


def _lowpass(fc, sample_rate, L):
    c, half, i0b = 2.0 * fc / float(sample_rate), 0.5 * float(L - 1), _i0(KAISER_BETA)
    h, total = [], 0.0
    for n in range(L):
        t = float(n) - half
        a = t / half if L > 1 else 0.0
        r = 1.0 - a * a
        w = _i0(KAISER_BETA * math.sqrt(r if r > 0.0 else 0.0)) / i0b
        arg = math.pi * c * t
        v = c * (1.0 if arg == 0.0 else math.sin(arg) / arg) * w
        h.append(v)
        total += v
    return np.array([v / total for v in h], np.float64)


def design(kind, sample_rate, f_lo, f_hi, n_taps):
    """float64 restatement of nae_fir_design (include/nae_gpu.h), not rounded"""
    delta = np.zeros(n_taps)
    delta[(n_taps - 1) // 2] = 1.0
    if kind == "lowpass":
        return _lowpass(f_hi, sample_rate, n_taps)
    if kind == "highpass":
        return delta - _lowpass(f_lo, sample_rate, n_taps)
    band = _lowpass(f_hi, sample_rate, n_taps) - _lowpass(f_lo, sample_rate, n_taps)
    return band if kind == "bandpass" else delta - band
