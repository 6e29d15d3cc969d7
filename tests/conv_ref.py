"""ctypes binding of the CPU statement of the long convolution (tests/conv_ref/ref_conv.c), built by tests/cstatement.py; the
library also holds the float64 restatement of the reverb design and, through its include, ref_fir_run."""
import ctypes as C
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "conv_ref", "ref_conv.c")
SIZES = (512, 1024, 2048, 4096)
MAX_TAPS, MAX_PARTS, PICK_PARTS = 262144, 512, 16      # NAE_CONV_MAX_TAPS, NAE_CONV_MAX_PARTS, NAE_CONV_PICK_PARTS


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_conv_pick_n_fft.argtypes = [C.c_int]
    L.ref_conv_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.ref_fir_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.ref_conv_reverb_taps.argtypes = [C.c_int, C.c_double, C.c_double]
    L.ref_conv_design_reverb.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int, C.c_void_p]
    L.ref_conv_design_reverb.restype = None
    return L


def parts(n_taps, n_fft):
    return -(-n_taps // (n_fft // 2))


def pick_n_fft(n_taps):
    """DESIGN.md §3, "K10 long convolution": the smallest supported N with at most 16 partitions, else 4096; 0 outside the limits"""
    if n_taps < 1 or n_taps > MAX_TAPS:
        return 0
    n = next((n for n in SIZES if parts(n_taps, n) <= PICK_PARTS), 4096)
    return n if parts(n_taps, n) <= MAX_PARTS else 0


def run(L, taps, n_fft, x, ch=1):
    """x: interleaved [n * ch] f32 -> interleaved [n * ch]; taps [n_taps] (every channel) or [ch][n_taps] (channel c its own)"""
    taps = np.ascontiguousarray(taps, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    n = x.size // ch
    for c in range(ch):
        h = taps if taps.ndim == 1 else np.ascontiguousarray(taps[c])
        rc = L.ref_conv_run(h.ctypes.data, h.size, n_fft, x.ctypes.data + 4 * c, n, ch, y.ctypes.data + 4 * c)
        assert rc == 0, rc
    return y


def run_streams(L, taps, n_fft, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, taps, n_fft, s.reshape(-1), ch=x.shape[2]).reshape(s.shape) for s in x])


def fir_run(L, taps, n_fft, x):
    """ref_fir_run (the FIR filter's statement) on one channel"""
    taps = np.ascontiguousarray(taps, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    rc = L.ref_fir_run(taps.ctypes.data, taps.size, n_fft, x.ctypes.data, x.size, 1, y.ctypes.data)
    assert rc == 0, rc
    return y


def direct(taps, x):
    """float64 causal convolution y[n] = sum_j h[j] x[n - j], n < len(x) (by FFT in double: the direct sum is too slow at these lengths)"""
    h, x = np.asarray(taps, np.float64), np.asarray(x, np.float64)
    n = 1 << int(np.ceil(np.log2(len(h) + len(x))))
    return np.fft.irfft(np.fft.rfft(h, n) * np.fft.rfft(x, n), n)[: len(x)]


def design_reverb(L, sample_rate, rt60, predelay, dry, wet, seed, n_taps=None):
    """the float64 restatement of nae_conv_design_reverb, not rounded"""
    if n_taps is None:
        n_taps = L.ref_conv_reverb_taps(sample_rate, rt60, predelay)
    h = np.zeros(n_taps, np.float64)
    L.ref_conv_design_reverb(sample_rate, rt60, predelay, dry, wet, seed, n_taps, h.ctypes.data)
    return h
