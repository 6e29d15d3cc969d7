"""ctypes binding of the CPU statement of the saturation (tests/sat_ref/ref_sat.c), built by tests/cstatement.py, a float64 numpy
restatement of it (zero-stuffing, np.convolve and the curve: no code shared with the statement) and of the design, and what the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sat_ref", "ref_sat.c")
CHUNK = 1024                    # NAE_EQ_CHUNK: the handle's unit
HALF, MAX_OS = 16, 8            # NAE_SAT_HALF, NAE_SAT_MAX_OS of include/nae_dsp_spec.h
SOFT, HARD = 0, 1
FACTORS = (1, 2, 4, 8)
INVALID, UNSUPPORTED = -1, -2   # NAE_ERR_INVALID, NAE_ERR_UNSUPPORTED


class Params(C.Structure):
    """nae_sat_params of include/nae_gpu.h"""
    _fields_ = [("oversample", C.c_int), ("curve", C.c_int), ("drive", C.c_float), ("bias", C.c_float), ("wet", C.c_float), ("dry", C.c_float)]


def params(oversample=4, curve=SOFT, drive=1.0, bias=0.0, wet=1.0, dry=0.0):
    p = Params()
    p.oversample, p.curve, p.drive, p.bias, p.wet, p.dry = oversample, curve, drive, bias, wet, dry
    return p


def as_tuple(p):
    return (p.oversample, p.curve, p.drive, p.bias, p.wet, p.dry)


def latency(m):
    return 0 if m == 1 else 2 * HALF


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_sat_latency.argtypes = [C.c_int]
    L.ref_sat_taps.argtypes = [C.c_int, C.c_void_p]
    L.ref_sat_check.argtypes = [C.POINTER(Params), C.c_int]
    L.ref_sat_design.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(Params)]
    L.ref_sat_curve.argtypes = [C.c_int, C.c_float]
    L.ref_sat_curve.restype = C.c_float
    L.ref_sat_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


def taps(L, m):
    """hd of the statement: 32 m + 1 taps, none at 1"""
    hd = np.zeros(2 * HALF * MAX_OS + 1, np.float32)
    n = L.ref_sat_taps(m, hd.ctypes.data)
    return hd[:n].copy()


def run(L, p, x):
    """x[n, ch] f32 -> y[n, ch] f32: the statement"""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[1] in (1, 2)
    y = np.zeros_like(x)
    rc = L.ref_sat_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data)
    assert rc == 0, rc
    return y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def run_tail(L, p, x):
    """what a handle delivers: the statement on x[n, ch] extended by the latency's zeros"""
    d = latency(p.oversample)
    return run(L, p, np.concatenate([x, np.zeros((d, x.shape[1]), np.float32)]))


def curve_np(curve, t):
    """the curve in float64"""
    if curve == SOFT:
        c = np.clip(t, -3.0, 3.0)
        return c * (27.0 + c * c) / (27.0 + 9.0 * c * c)
    return np.clip(t, -1.0, 1.0)


def run_np(p, x, hd):
    """float64 restatement: zero-stuff by M, convolve with M hd, shape, convolve with hd, keep every M-th sample, mix with the delayed
    input.  hd: the taps (f32 values, used in float64).  x[n, ch] -> y[n, ch] float64"""
    x = np.asarray(x, np.float64)
    n, ch = x.shape
    m = p.oversample
    g, b, wet, dry = (np.float64(v) for v in (p.drive, p.bias, p.wet, p.dry))
    fb = curve_np(p.curve, b)
    y = np.zeros((n, ch))
    for c in range(ch):
        if m == 1:
            y[:, c] = dry * x[:, c] + wet * (curve_np(p.curve, g * x[:, c] + b) - fb)
            continue
        h = np.asarray(hd, np.float64)
        up = np.zeros(n * m)
        up[::m] = x[:, c]
        u = np.convolve(up, m * h)[:n * m]
        v = curve_np(p.curve, g * u + b) - fb
        s = np.convolve(v, h)[:n * m][::m]
        delayed = np.concatenate([np.zeros(2 * HALF), x[:, c]])[:n]
        y[:, c] = dry * delayed + wet * s
    return y


def design(drive_db=12.0, bias=0.0, curve=SOFT, oversample=4, output_db=0.0, mix=1.0):
    """float64 restatement of nae_sat_design (include/nae_gpu.h), each field rounded once; the library's error code where it refuses"""
    if not all(math.isfinite(a) for a in (drive_db, bias, output_db, mix)):
        return INVALID
    if not (0.0 <= drive_db <= 48.0 and 0.0 <= bias <= 1.0 and -24.0 <= output_db <= 24.0 and 0.0 <= mix <= 1.0) or curve not in (SOFT, HARD):
        return INVALID
    if oversample not in FACTORS:
        return UNSUPPORTED
    f32 = np.float32
    return params(oversample, curve, float(f32(10.0 ** (drive_db / 20.0))), float(f32(bias)), float(f32(mix * 10.0 ** (output_db / 20.0))),
                  float(f32(1.0 - mix)))
