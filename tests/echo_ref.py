"""ctypes binding of the CPU statement of the echo (tests/echo_ref/ref_echo.c), built by tests/cstatement.py, a float64 numpy restatement of
its sequential form and of the design, and the parameter sets the tests share.  The library holds the equalizer's statement too (the file
includes it), so tests/eq_ref.py's functions run on it."""
import ctypes as C
import math
import os

import numpy as np

import cstatement
import eq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "echo_ref", "ref_echo.c")
CHUNK = eq_ref.CHUNK
MIN_DELAY, MAX_DELAY, MAX_SECTIONS, MAX_FEEDBACK = CHUNK, 1 << 20, 4, 0.99   # NAE_ECHO_* of include/nae_dsp_spec.h


class Params(C.Structure):
    """nae_echo_params of include/nae_gpu.h"""
    _fields_ = [("delay", C.c_int * 2), ("feedback", C.c_double), ("cross", C.c_int), ("wet", C.c_double), ("dry", C.c_double),
                ("n_sections", C.c_int), ("coef", (C.c_double * 5) * MAX_SECTIONS)]


def params(delay, feedback=0.5, cross=0, wet=1.0, dry=1.0, coef=(), n_sections=None):
    """delay: samples, one number or (left, right); coef: [n][5]; n_sections: a count that differs from len(coef), for the rejections"""
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    left, right = (delay, delay) if np.isscalar(delay) else delay
    p = Params()
    p.delay[0], p.delay[1] = int(left), int(right)
    p.feedback, p.cross, p.wet, p.dry = feedback, int(cross), wet, dry
    p.n_sections = coef.shape[0] if n_sections is None else n_sections
    for s, row in enumerate(coef[:MAX_SECTIONS]):
        for i, v in enumerate(row):
            p.coef[s][i] = v
    return p


def coef_of(p):
    return np.array([[p.coef[s][i] for i in range(5)] for s in range(max(0, min(p.n_sections, MAX_SECTIONS)))], np.float64).reshape(-1, 5)


def as_tuple(p):
    """the record's scalar fields and its sections, for comparing two records"""
    return (p.delay[0], p.delay[1], p.feedback, p.cross, p.wet, p.dry, p.n_sections, coef_of(p).tobytes())


def ring(p, ch):
    """R: the smallest multiple of the chunk that holds the call's longest delay and one chunk ("K16 echo")"""
    d = max(p.delay[0], p.delay[1]) if ch == 2 else p.delay[0]
    return (d + 2 * CHUNK - 1) // CHUNK * CHUNK


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_echo_check.argtypes = [C.POINTER(Params), C.c_int]
    L.ref_echo_design.argtypes = [C.c_int] + [C.c_double] * 7 + [C.c_int, C.POINTER(Params)]
    L.ref_echo_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    # the statement it includes, under its own binding's types
    for name in ("ref_eq_run", "ref_eq_run_f64", "ref_eq_sequential"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    return L


def _run(L, p, x, tiled, want_line=False):
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[1] in (1, 2)
    y, line = np.zeros_like(x), np.zeros_like(x)
    rc = L.ref_echo_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, tiled, line.ctypes.data if want_line else None)
    assert rc == 0, rc
    return (y, line) if want_line else y


def run(L, p, x, want_line=False):
    """x[n, ch] f32 -> y[n, ch] f32 (and the line w[n, ch]): the tiled statement, what the GPU computes"""
    return _run(L, p, x, 1, want_line)


def sequential(L, p, x, want_line=False):
    """the same formulas with the sections' direct-form recurrence sample by sample; the line still f32"""
    return _run(L, p, x, 0, want_line)


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def sequential_np(p, x):
    """float64 numpy restatement of the sequential form: every step one float64 operation in the specification's order, the line np.float32"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    f64, f32 = np.float64, np.float32
    coef = coef_of(p)
    g, wet, dry = f64(p.feedback), f64(p.wet), f64(p.dry)
    w, y = np.zeros((n, ch), f32), np.zeros((n, ch), f32)
    z = np.zeros((ch, max(len(coef), 1), 2), f64)
    D = [p.delay[c] for c in range(ch)]
    src = [1 - c if p.cross and ch == 2 else c for c in range(ch)]
    for i in range(n):
        for c in range(ch):
            fv = f64(w[i - D[c], src[c]]) if i >= D[c] else f64(0.0)
            for s, (b0, b1, b2, a1, a2) in enumerate(coef):
                yv = b0 * fv + z[c, s, 0]
                z[c, s, 0] = (b1 * fv - a1 * yv) + z[c, s, 1]
                z[c, s, 1] = b2 * fv - a2 * yv
                fv = yv
            xd = f64(x[i, c])
            w[i, c] = f32(xd + (g * fv))
            y[i, c] = f32((dry * xd) + (wet * fv))
    return y


def design(sample_rate, delay_s_left, delay_s_right, feedback, damp_hz=0.0, lowcut_hz=0.0, wet=0.35, dry=1.0, cross=0):
    """float64 restatement of nae_echo_design (include/nae_gpu.h): the delays to the nearest sample (halves away from zero, as lround), a
    low-pass at damp_hz and then a high-pass at lowcut_hz by tests/eq_ref.design at q = sqrt(1 / 2); None where the library answers
    NAE_ERR_INVALID"""
    args = (delay_s_left, delay_s_right, feedback, damp_hz, lowcut_hz, wet, dry)
    if sample_rate <= 0 or cross not in (0, 1) or not all(math.isfinite(a) for a in args):
        return None
    if not abs(feedback) <= MAX_FEEDBACK or damp_hz < 0.0 or lowcut_hz < 0.0:
        return None
    delays = []
    for d in (np.float64(delay_s_left) * np.float64(sample_rate), np.float64(delay_s_right) * np.float64(sample_rate)):
        r = math.floor(float(d) + 0.5)
        if not MIN_DELAY <= r <= MAX_DELAY:
            return None
        delays.append(r)
    coef = []
    for kind, hz in (("lowpass", damp_hz), ("highpass", lowcut_hz)):
        if hz > 0.0:
            if not hz < 0.5 * sample_rate:
                return None
            coef.append(eq_ref.design(kind, sample_rate, hz, 0.0, math.sqrt(0.5)))
    return params(tuple(delays), feedback, cross, wet, dry, coef)


def loop_filters(sample_rate=48000):
    """the loop filters the tests share, by section count: none, a damping low-pass, the designed pair (low-pass and low cut), and four
    sections (two of each: a steeper band); every one Butterworth, gain at most 1"""
    lp = lambda hz: eq_ref.design("lowpass", sample_rate, hz, 0.0, math.sqrt(0.5))
    hp = lambda hz: eq_ref.design("highpass", sample_rate, hz, 0.0, math.sqrt(0.5))
    return {0: np.zeros((0, 5)), 1: lp(4000.0).reshape(1, 5), 2: np.stack([lp(4000.0), hp(150.0)]),
            4: np.stack([lp(6000.0), hp(100.0), lp(9000.0), hp(40.0)])}
