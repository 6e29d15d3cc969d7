"""ctypes binding of the CPU statement of the biquad cascade (tests/eq_ref/ref_eq.c), built by tests/cstatement.py, the float64
restatement of the design, the magnitude of a cascade from its coefficients, and the cascades the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "eq_ref", "ref_eq.c")
LANE, CHUNK, MAX_SECTIONS = 16, 1024, 16               # NAE_EQ_LANE, NAE_EQ_CHUNK, NAE_EQ_MAX_SECTIONS
KINDS = ("peak", "lowshelf", "highshelf", "lowpass", "highpass", "notch")   # NAE_EQ_PEAK ... NAE_EQ_NOTCH = 0 ... 5

# (b0, b1, b2, a1, a2): on and outside the stability triangle |a2| < 1, |a1| < 1 + a2, and non-finite
BAD_SECTIONS = ((1, 0, 0, 0, 1.0), (1, 0, 0, 0, -1.0), (1, 0, 0, 0, 1.5), (1, 0, 0, 1.5, 0.5), (1, 0, 0, -1.5, 0.5), (1, 0, 0, 2.0, 0.999),
                (1, 0, 0, -0.2, -0.9), (float("nan"), 0, 0, 0, 0), (1, float("inf"), 0, 0, 0), (1, 0, -float("inf"), 0, 0),
                (1, 0, 0, float("nan"), 0), (1, 0, 0, 0, float("nan")))
GOOD_SECTIONS = ((1, 0, 0, 0, 0), (1, 0, 0, 1.499, 0.5), (1, 0, 0, 0, 0.999), (1, 0, 0, 0, -0.999), (1e6, -1e6, 3, -1.9, 0.95))


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_eq_check.argtypes = [C.c_void_p, C.c_int]
    for name in ("ref_eq_run", "ref_eq_run_f64", "ref_eq_sequential", "ref_eq_sequential_f32", "ref_eq_sequential_ld"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.ref_eq_design.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.ref_eq_tables.argtypes, L.ref_eq_tables.restype = [C.c_double, C.c_double, C.c_void_p], None
    return L


def _coef(coef):
    coef = np.ascontiguousarray(coef, np.float64).reshape(-1, 5)
    return coef, coef.shape[0]


def run(L, coef, x, ch=1):
    """x: interleaved [n * ch] f32 -> interleaved [n * ch], every channel through the cascade coef[S][5]; the tiled statement"""
    coef, S = _coef(coef)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    for c in range(ch):
        rc = L.ref_eq_run(coef.ctypes.data, S, x.ctypes.data + 4 * c, x.size // ch, ch, y.ctypes.data + 4 * c)
        assert rc == 0, rc
    return y


def run_f64(L, coef, x):
    """the tiled statement on one channel in front of its final rounding"""
    coef, S = _coef(coef)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.size, np.float64)
    assert L.ref_eq_run_f64(coef.ctypes.data, S, x.ctypes.data, x.size, 1, y.ctypes.data) == 0
    return y


def run_streams(L, coef, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, coef, s.reshape(-1), ch=x.shape[2]).reshape(s.shape) for s in x])


def sequential(L, coef, x):
    """the plain sequential double recurrence on one channel, not rounded"""
    coef, S = _coef(coef)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.size, np.float64)
    assert L.ref_eq_sequential(coef.ctypes.data, S, x.ctypes.data, x.size, 1, y.ctypes.data) == 0
    return y


def sequential_f32(L, coef, x):
    """the same recurrence with every value in f32"""
    coef, S = _coef(coef)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.size, np.float32)
    assert L.ref_eq_sequential_f32(coef.ctypes.data, S, x.ctypes.data, x.size, 1, y.ctypes.data) == 0
    return y


def sequential_ld(L, coef, x):
    """the same recurrence with every value in long double, returned as double: the truth of the steady-state tests"""
    coef, S = _coef(coef)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.size, np.float64)
    assert L.ref_eq_sequential_ld(coef.ctypes.data, S, x.ctypes.data, x.size, 1, y.ctypes.data) == 0
    return y


def ldbl_mant_dig(L):
    """the significand bits of the statement's long double"""
    return L.ref_eq_ldbl_mant_dig()


def tables(L, a1, a2):
    """the statement's tables of one section in the library's block order: p[16] q[16] Phi_0 ... Phi_5, each m00 m01 m10 m11"""
    out = np.zeros(2 * LANE + 24, np.float64)
    L.ref_eq_tables(float(a1), float(a2), out.ctypes.data)
    return out


def design(kind, sample_rate, freq, gain_db=0.0, q=0.7071):
    """float64 restatement of nae_eq_design (include/nae_gpu.h): numpy float64 arithmetic; sin, cos, sqrt and the power come from libm through
    `math`, as the library's do (numpy's own vector routines may differ from libm in the last place, and 1 - cos w0 at 20 Hz magnifies that)"""
    f = np.float64
    A = f(math.pow(10.0, float(f(gain_db) / f(40.0))))
    w0 = f(2.0) * f(math.pi) * f(freq) / f(sample_rate)
    cs, alpha = f(math.cos(w0)), f(math.sin(w0)) / (f(2.0) * f(q))
    r = f(2.0) * f(math.sqrt(A)) * alpha
    one, two = f(1.0), f(2.0)
    if kind == "peak":
        b = (one + alpha * A, -two * cs, one - alpha * A)
        a = (one + alpha / A, -two * cs, one - alpha / A)
    elif kind == "lowshelf":
        b = (A * ((A + one) - (A - one) * cs + r), two * A * ((A - one) - (A + one) * cs), A * ((A + one) - (A - one) * cs - r))
        a = ((A + one) + (A - one) * cs + r, -two * ((A - one) + (A + one) * cs), (A + one) + (A - one) * cs - r)
    elif kind == "highshelf":
        b = (A * ((A + one) + (A - one) * cs + r), -two * A * ((A - one) + (A + one) * cs), A * ((A + one) + (A - one) * cs - r))
        a = ((A + one) - (A - one) * cs + r, two * ((A - one) - (A + one) * cs), (A + one) - (A - one) * cs - r)
    else:
        a = (one + alpha, -two * cs, one - alpha)
        if kind == "lowpass":
            b = ((one - cs) / two, one - cs, (one - cs) / two)
        elif kind == "highpass":
            b = ((one + cs) / two, -(one + cs), (one + cs) / two)
        else:
            assert kind == "notch", kind
            b = (one, -two * cs, one)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], np.float64)


def stable(coef):
    """the library's rule: |a2| < 1 and |a1| < 1 + a2, every coefficient finite"""
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    return bool(np.all(np.isfinite(coef)) and np.all(np.abs(coef[:, 4]) < 1.0) and np.all(np.abs(coef[:, 3]) < 1.0 + coef[:, 4]))


def magnitude_db(coef, freq, sample_rate):
    """|H(e^jw)| of the cascade in dB, from the coefficients"""
    z = np.exp(-2j * np.pi * freq / sample_rate)
    h = 1.0 + 0j
    for b0, b1, b2, a1, a2 in np.asarray(coef, np.float64).reshape(-1, 5):
        h *= (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return 20.0 * np.log10(max(abs(h), 1e-300))


def hard_cascade(sample_rate=48000):
    """16 sections, four of them 20 Hz / Q 10 / +12 dB bells ("K11 biquad cascade"): long, badly conditioned responses"""
    bands = [("peak", 20.0, 12.0, 10.0)] * 4 + [("highpass", 30.0, 0.0, 0.7071), ("lowshelf", 120.0, -6.0, 0.7071), ("peak", 60.0, -9.0, 8.0),
                                                ("peak", 250.0, 4.0, 1.4), ("peak", 1000.0, -3.0, 2.0), ("peak", 3150.0, 6.0, 4.0),
                                                ("notch", 50.0, 0.0, 30.0), ("peak", 8000.0, -12.0, 0.5), ("highshelf", 10000.0, 5.0, 0.7071),
                                                ("lowpass", 18000.0, 0.0, 0.7071), ("peak", 40.0, 24.0, 40.0), ("peak", 15000.0, -24.0, 0.1)]
    return np.stack([design(k, sample_rate, f, g, q) for k, f, g, q in bands])


def cascade(n_sections, sample_rate=48000):
    """the first n_sections of a cascade that ends in the hard one's bells: S = 16 is the hard cascade, in another order"""
    h = hard_cascade(sample_rate)
    order = [5, 7, 0, 9, 4, 8, 1, 10, 12, 6, 2, 11, 13, 3, 14, 15]
    return np.ascontiguousarray(h[order[:n_sections]])
