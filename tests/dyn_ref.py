"""ctypes binding of the CPU statement of the dynamics processor (tests/dyn_ref/ref_dyn.c), built by tests/cstatement.py, the float64
restatements of the design and of the static curve, and the parameter sets the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dyn_ref", "ref_dyn.c")
LANE, CHUNK, MAX_LOOKAHEAD, FLOOR_DB = 16, 1024, 1024, -1000.0   # NAE_DYN_LANE, NAE_DYN_CHUNK, NAE_DYN_MAX_LOOKAHEAD, NAE_DYN_FLOOR_DB
K = 20.0 * math.log10(2.0)


class Params(C.Structure):
    """nae_dyn_params of include/nae_gpu.h"""
    _fields_ = [("threshold_db", C.c_double), ("slope", C.c_double), ("knee_db", C.c_double), ("alpha_attack", C.c_double),
                ("alpha_release", C.c_double), ("makeup_db", C.c_double), ("lookahead", C.c_int), ("link", C.c_int)]


def params(threshold_db=-18.0, slope=0.75, knee_db=6.0, alpha_attack=0.9, alpha_release=0.999, makeup_db=0.0, lookahead=0, link=1):
    return Params(threshold_db, slope, knee_db, alpha_attack, alpha_release, makeup_db, lookahead, link)


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in Params._fields_)


def alpha(t, sample_rate=48000):
    return math.exp(-1.0 / (t * sample_rate)) if t > 0 else 0.0


# the fastest and the slowest smoothing nae_dyn_design makes at 48 kHz: attack 0 / release 1 ms, and attack 0.5 s / release 5 s
FAST = dict(alpha_attack=0.0, alpha_release=alpha(0.001))
SLOW = dict(alpha_attack=alpha(0.5), alpha_release=alpha(5.0))


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_dyn_check.argtypes = [C.POINTER(Params)]
    L.ref_dyn_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_dyn_run_f64.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_dyn_sequential.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.ref_dyn_design.argtypes = [C.c_int] + [C.c_double] * 7 + [C.c_int, C.POINTER(Params)]
    for name in ("ref_dyn_log2_v", "ref_dyn_exp2_v"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def run(L, p, x):
    """x[n, ch] f32 -> [n, ch] f32: the tiled statement"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    assert L.ref_dyn_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data) == 0
    return y


def run_f64(L, p, x):
    """the tiled statement in front of its final rounding"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.shape, np.float64)
    assert L.ref_dyn_run_f64(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data) == 0
    return y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def sequential(L, p, x, with_yl=False):
    """the plain sequential double recurrence, not rounded; with_yl: also the smoothed reduction [n, detectors]"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(x.shape, np.float64)
    n_det = 1 if (p.link and x.shape[1] == 2) else x.shape[1]
    yl = np.zeros((x.shape[0], n_det), np.float64)
    assert L.ref_dyn_sequential(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, yl.ctypes.data) == 0
    return (y, yl) if with_yl else y


def log2_v(L, a):
    a = np.ascontiguousarray(a, np.float64)
    out = np.empty_like(a)
    L.ref_dyn_log2_v(a.ctypes.data, a.size, out.ctypes.data)
    return out


def exp2_v(L, t):
    t = np.ascontiguousarray(t, np.float64)
    out = np.empty_like(t)
    L.ref_dyn_exp2_v(t.ctypes.data, t.size, out.ctypes.data)
    return out


def design(sample_rate, threshold_db, ratio, knee_db, attack_s, release_s, lookahead_s, makeup_db, link):
    """float64 restatement of nae_dyn_design (include/nae_gpu.h): numpy float64 arithmetic with libm's exp through `math`, as the library's
    (numpy's vector exp may differ from libm in the last place)"""
    f = np.float64
    slope = f(1.0) if math.isinf(ratio) else f(1.0) - f(1.0) / f(ratio)
    a_att = f(math.exp(float(f(-1.0) / (f(attack_s) * f(sample_rate))))) if attack_s > 0 else f(0.0)
    a_rel = f(math.exp(float(f(-1.0) / (f(release_s) * f(sample_rate)))))
    la = int(math.floor(float(f(lookahead_s) * f(sample_rate)) + 0.5))          # lround of a value that is not negative
    return Params(threshold_db, slope, knee_db, a_att, a_rel, makeup_db, la, int(link))


def demand_db(p, level_db):
    """the static curve's gain-reduction demand in float64 from a level in dB: what a compressor's text book says"""
    u = level_db - p.threshold_db
    if 2.0 * u < -p.knee_db:
        return 0.0
    if p.knee_db > 0 and abs(2.0 * u) <= p.knee_db:
        return p.slope * (u + p.knee_db / 2.0) ** 2 / (2.0 * p.knee_db)
    return p.slope * u


def signals(n, threshold_db=-18.0, seed=1):
    """[n, 2] f32 each: noise whose level wanders +-12 dB around the threshold, a two-tone, and a train of bursts"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    lvl = 10.0 ** ((threshold_db + 12.0 * np.sin(2 * np.pi * t / 1777.0)) / 20.0)
    noise = (rng.uniform(-1, 1, (n, 2)) * lvl[:, None] * np.sqrt(3.0)).astype(np.float32)
    tone = 0.6 * np.sin(2 * np.pi * 0.0371 * t) + 0.3 * np.sin(2 * np.pi * 0.213 * t + 1.0)
    two = np.stack([tone, 0.5 * np.roll(tone, 37)], 1).astype(np.float32)
    burst = (rng.uniform(-1, 1, (n, 2)) * np.where((t % 700) < 90, 0.9, 0.003)[:, None]).astype(np.float32)
    return {"noise": noise, "two-tone": two, "bursts": burst}
