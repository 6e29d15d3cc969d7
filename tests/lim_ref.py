"""ctypes binding of the CPU statement of the limiter (tests/lim_ref/ref_lim.c), built by tests/cstatement.py, a float64 numpy restatement of
the limiter and of its design that shares no code with the C, and the parameter sets and signals the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement
import loud_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lim_ref", "ref_lim.c")
LANE, CHUNK, FLOOR_DB = 16, 1024, -1000.0        # NAE_DYN_LANE, NAE_DYN_CHUNK, NAE_DYN_FLOOR_DB
REACH, MAX_LOOKAHEAD = 6, 1018                    # NAE_LIM_TP_REACH, NAE_LIM_MAX_LOOKAHEAD
Q_SCALE = 16777216.0                              # NAE_LIM_Q_SCALE
K = 20.0 * math.log10(2.0)
RATE = 48000
CEILING_SLACK = 1.0 + 2.0 ** -22                  # DESIGN.md §3, "K22 limiter", "Sample ceiling": derived, not measured


class Params(C.Structure):
    """nae_lim_params of include/nae_gpu.h"""
    _fields_ = [("ceiling_db", C.c_double), ("gain_db", C.c_double), ("alpha_release", C.c_double), ("lookahead", C.c_int),
                ("true_peak", C.c_int), ("link", C.c_int)]


def alpha(t, sample_rate=RATE):
    return math.exp(-1.0 / (t * sample_rate))


FAST, SLOW = alpha(0.001), alpha(5.0)             # the fastest and the slowest release nae_lim_design makes at 48 kHz


def params(ceiling_db=-1.0, gain_db=12.0, alpha_release=FAST, lookahead=72, true_peak=1, link=1):
    return Params(ceiling_db, gain_db, alpha_release, lookahead, true_peak, link)


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in Params._fields_)


def copy(p, **changes):
    q = Params.from_buffer_copy(p)
    for k, v in changes.items():
        setattr(q, k, v)
    return q


def reach(p):
    """D: the samples past n the level of n reads"""
    return REACH if p.true_peak else 0


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_lim_check.argtypes = [C.POINTER(Params)]
    L.ref_lim_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_lim_full.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * 6
    L.ref_lim_design.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_int, C.POINTER(Params)]
    return L


def run(L, p, x):
    """x[n, ch] f32 -> [n, ch] f32: the tiled statement"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    assert L.ref_lim_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data) == 0
    return y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def full(L, p, x, tiled):
    """either form with everything it makes: dict of y (f32), yd (f64, not rounded) and, [n, detectors] each, r (the demand), s (the smoothed
    reduction), y1 (the release's output) and w (the integer window sums)"""
    x = np.ascontiguousarray(x, np.float32)
    n_det = 1 if (p.link and x.shape[1] == 2) else x.shape[1]
    shape = (x.shape[0], n_det)
    out = dict(y=np.zeros_like(x), yd=np.zeros(x.shape, np.float64), r=np.zeros(shape, np.float64), s=np.zeros(shape, np.float64),
               y1=np.zeros(shape, np.float64), w=np.zeros(shape, np.int64))
    assert L.ref_lim_full(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], int(tiled), out["y"].ctypes.data, out["yd"].ctypes.data,
                          out["r"].ctypes.data, out["s"].ctypes.data, out["y1"].ctypes.data, out["w"].ctypes.data) == 0
    return out


def design(sample_rate, ceiling_db, gain_db, release_s, lookahead_s, true_peak, link):
    """float64 restatement of nae_lim_design (include/nae_gpu.h): numpy float64 arithmetic with libm's exp through `math`, as the library's"""
    f = np.float64
    a_rel = f(math.exp(float(f(-1.0) / (f(release_s) * f(sample_rate)))))
    la = int(math.floor(float(f(lookahead_s) * f(sample_rate)) + 0.5))          # lround of a value that is not negative
    return Params(ceiling_db, gain_db, a_rel, la, int(true_peak), int(link))


def restate(p, x):
    """the limiter in numpy float64 from the specification's text, sharing no code with the C: np.convolve with unrounded taps, np.log2 and
    np.exp2, maxima and sums of windows from shifted arrays and cumulative sums, the plain recurrence -> dict of yd [n, ch] and, [n,
    detectors] each, r and s"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    linked = bool(p.link) and ch == 2
    groups = [(0, 1)] if linked else [(c,) for c in range(ch)]
    la = p.lookahead
    ext = n + la                                                                 # the demand is read up to n - 1 + la
    yd = np.zeros((n, ch), np.float64)
    r_all, s_all = np.zeros((n, len(groups))), np.zeros((n, len(groups)))
    taps = loud_ref.taps64()
    for gi, cols in enumerate(groups):
        level = np.zeros(ext)
        for c in cols:
            xc = np.zeros(ext + 8)
            xc[:n] = x[:, c].astype(np.float64)
            lc = np.abs(xc[:ext])
            if p.true_peak:
                e = np.max(np.abs(np.stack([np.convolve(xc, t)[:ext + 8] for t in taps])), axis=0)   # e[m], m = 0 ... ext + 7
                lc = np.maximum(lc, np.maximum(e[5:ext + 5], e[6:ext + 6]))
            level = np.maximum(level, lc)
        with np.errstate(divide="ignore"):
            xg = np.where(level == 0, FLOOR_DB, K * np.log2(level))
        r = np.maximum(xg + p.gain_db - p.ceiling_db, 0.0)
        d = r[:n].copy()
        for t in range(1, la + 1):
            np.maximum(d, r[t:t + n], out=d)
        y1 = np.empty(n)
        prev, ar = 0.0, p.alpha_release
        omr = 1.0 - ar
        for k in range(n):
            prev = max(d[k], ar * prev + omr * d[k])
            y1[k] = prev
        q = np.ceil(y1 * Q_SCALE)
        qq = np.concatenate([np.full(la + 1, q[0]), q])                          # q[n] = q[0] below 0
        cs = np.cumsum(qq)                                                       # exact in float64: integers under 2^53
        s = (cs[la + 1:] - cs[:n]) / ((la + 1) * Q_SCALE)
        g = np.exp2((p.gain_db - s) / K)
        r_all[:, gi], s_all[:, gi] = r[:n], s
        for c in cols:
            yd[:, c] = x[:, c].astype(np.float64) * g
    return dict(yd=yd, r=r_all, s=s_all)


def true_peak_db(y):
    """the largest true peak over y's channels in dBTP, by the float64 restatement of K14's meter (tests/loud_ref.py)"""
    return 20.0 * math.log10(max(loud_ref.true_peak_at(y[:, c])[1] for c in range(y.shape[1])))


PEAKS = (1017, 1018, 1023, 1024, 1029, 1035, 2047, 3078)
SIGNALS = ("fs4", "noise", "bursts", "high", "peaks")


def signals(n=3 * CHUNK + 7, seed=1):
    """[n, 2] f32 each, at 48 kHz: K14's fs/4 sine whose samples all lie 3 dB under its peak, uniform noise, a 997 Hz burst train between
    -40 dB rests, a sine at 0.4 fs, and single full-scale samples at PEAKS (where they lie inside n): the FIR's 11 behind, its 6 ahead and
    the window all cross chunk borders and the signal's end"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    fs4 = 0.5 * np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)
    tone = np.sin(2 * np.pi * 997.0 * t / RATE)
    burst = tone * np.where((t % 700) < 180, 0.9, 0.01)
    high = 0.7 * np.sin(2 * np.pi * 0.4 * t + 0.3)
    peaks = np.zeros((n, 2))
    for i, at in enumerate(at for at in PEAKS if at < n):
        peaks[at, i % 2] = 1.0 if i % 3 else -1.0
    peaks += 1e-3 * rng.uniform(-1, 1, (n, 2))
    return {"fs4": np.stack([fs4, 0.8 * fs4], 1).astype(np.float32), "noise": rng.uniform(-1, 1, (n, 2)).astype(np.float32),
            "bursts": np.stack([burst, 0.7 * np.roll(burst, 91)], 1).astype(np.float32),
            "high": np.stack([high, np.roll(high, 3)], 1).astype(np.float32), "peaks": peaks.astype(np.float32)}
