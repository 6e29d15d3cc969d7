"""ctypes binding of the CPU statement of the gate (tests/gate_ref/ref_gate.c), built by tests/cstatement.py, a float64 numpy restatement of
the gate and of its design that shares no code with the C, and the parameter sets and signals the tests share."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gate_ref", "ref_gate.c")
LANE, CHUNK, MAX_LOOKAHEAD, FLOOR_DB = 16, 1024, 1024, -1000.0   # NAE_DYN_LANE, NAE_DYN_CHUNK, NAE_DYN_MAX_LOOKAHEAD, NAE_DYN_FLOOR_DB
MAX_HOLD = 1 << 21                                                # NAE_GATE_MAX_HOLD
K = 20.0 * math.log10(2.0)
MODES = ("gate", "expander")


class Params(C.Structure):
    """nae_gate_params of include/nae_gpu.h"""
    _fields_ = [("open_lin", C.c_float), ("close_lin", C.c_float), ("threshold_db", C.c_double), ("slope", C.c_double), ("range_db", C.c_double),
                ("alpha_attack", C.c_double), ("alpha_release", C.c_double), ("hold", C.c_int), ("lookahead", C.c_int), ("expand", C.c_int),
                ("link", C.c_int)]


def alpha(t, sample_rate=48000):
    return math.exp(-1.0 / (t * sample_rate)) if t > 0 else 0.0


# the fastest and the slowest smoothing nae_gate_design makes at 48 kHz: attack 0 / release 1 ms, and attack 0.5 s / release 5 s
FAST = dict(alpha_attack=0.0, alpha_release=alpha(0.001))
SLOW = dict(alpha_attack=alpha(0.5), alpha_release=alpha(5.0))


def params(threshold_db=-30.0, hysteresis_db=6.0, slope=1.0, range_db=60.0, alpha_attack=0.9, alpha_release=0.999, hold=0, lookahead=0, expand=0,
           link=1, open_lin=None, close_lin=None):
    """a record with the thresholds made from decibels, or given as magnitudes"""
    o = np.float32(10.0 ** (threshold_db / 20.0)) if open_lin is None else np.float32(open_lin)
    c = np.float32(10.0 ** ((threshold_db - hysteresis_db) / 20.0)) if close_lin is None else np.float32(close_lin)
    return Params(o, c, threshold_db, slope, range_db, alpha_attack, alpha_release, hold, lookahead, expand, link)


def as_tuple(p):
    return tuple(getattr(p, f) for f, _ in Params._fields_)


def copy(p, **changes):
    q = Params.from_buffer_copy(p)
    for k, v in changes.items():
        setattr(q, k, v)
    return q


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_gate_check.argtypes = [C.POINTER(Params)]
    L.ref_gate_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_gate_full.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * 5
    L.ref_gate_design.argtypes = [C.c_int, C.c_int] + [C.c_double] * 8 + [C.c_int, C.POINTER(Params)]
    return L


def run(L, p, x):
    """x[n, ch] f32 -> [n, ch] f32: the tiled statement"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    assert L.ref_gate_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data) == 0
    return y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def full(L, p, x, tiled):
    """either form with everything it makes: dict of y (f32), yd (f64, not rounded), sm (the smoothed depth), s and open ([n, detectors])"""
    x = np.ascontiguousarray(x, np.float32)
    n_det = 1 if (p.link and x.shape[1] == 2) else x.shape[1]
    out = dict(y=np.zeros_like(x), yd=np.zeros(x.shape, np.float64), sm=np.zeros((x.shape[0], n_det), np.float64),
               s=np.zeros((x.shape[0], n_det), np.uint8), open=np.zeros((x.shape[0], n_det), np.uint8))
    assert L.ref_gate_full(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], int(tiled), out["y"].ctypes.data, out["yd"].ctypes.data,
                           out["sm"].ctypes.data, out["s"].ctypes.data, out["open"].ctypes.data) == 0
    return out


def design(sample_rate, mode, threshold_db, hysteresis_db, range_db, ratio, attack_s, hold_s, release_s, lookahead_s, link):
    """float64 restatement of nae_gate_design (include/nae_gpu.h): numpy float64 arithmetic with libm's exp and pow through `math`, as the
    library's (numpy's vector functions may differ from libm in the last place)"""
    f = np.float64
    o = np.float32(math.pow(10.0, float(f(threshold_db) / f(20.0))))
    c = np.float32(math.pow(10.0, float((f(threshold_db) - f(hysteresis_db)) / f(20.0))))
    a_att = f(math.exp(float(f(-1.0) / (f(attack_s) * f(sample_rate))))) if attack_s > 0 else f(0.0)
    a_rel = f(math.exp(float(f(-1.0) / (f(release_s) * f(sample_rate)))))
    la = int(math.floor(float(f(lookahead_s) * f(sample_rate)) + 0.5))          # lround of a value that is not negative
    hd = int(math.floor(float(f(hold_s) * f(sample_rate)) + 0.5))
    return Params(o, c, threshold_db, f(ratio) - f(1.0), range_db, a_att, a_rel, hd, la, MODES.index(mode), int(link))


def restate(p, x):
    """the gate in numpy float64 from the specification's text, sharing no code with the C: the hysteresis by the index of the last event,
    window membership from cumulative sums, np.log2 and np.exp2, the plain recurrence -> dict of open [n, detectors] and yd [n, ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    linked = bool(p.link) and ch == 2
    groups = [(0, 1)] if linked else [(c,) for c in range(ch)]
    open_all = np.zeros((n, len(groups)), np.uint8)
    yd = np.zeros((n, ch), np.float64)
    la, hold = p.lookahead, p.hold
    for gi, cols in enumerate(groups):
        a = np.abs(x[:, cols[0]])
        if len(cols) == 2:
            b = np.abs(x[:, cols[1]])
            a = np.where(b > a, b, a)
        with np.errstate(invalid="ignore"):
            setv, clr = a >= np.float32(p.open_lin), a < np.float32(p.close_lin)
        idx = np.where(setv | clr, np.arange(n), -1)
        lastev = np.maximum.accumulate(idx)
        s = np.where(lastev >= 0, setv[np.maximum(lastev, 0)], False)
        cs = np.concatenate([[0], np.cumsum(s.astype(np.int64))])                # cs[k] = set samples below k
        i = np.arange(n)
        hi = np.minimum(i + la + 1, n)
        lo = np.maximum(i - hold, 0)
        is_open = (cs[hi] - cs[lo]) > 0
        open_all[:, gi] = is_open
        if p.expand:
            with np.errstate(divide="ignore", invalid="ignore"):
                xg = np.where(a == 0, FLOOR_DB, K * np.log2(a.astype(np.float64)))
                u = p.threshold_db - xg
                v = p.slope * u
                depth = np.where(u <= 0, 0.0, np.where(v < p.range_db, v, p.range_db))
        else:
            depth = np.full(n, p.range_db)
        al = np.where(is_open, p.alpha_attack, p.alpha_release)
        bb = np.where(is_open, 0.0, (1.0 - p.alpha_release) * depth)
        y = np.empty(n)
        prev = p.range_db
        for k in range(n):
            prev = al[k] * prev + bb[k]
            y[k] = prev
        g = np.exp2(-y / K)
        for c in cols:
            yd[:, c] = x[:, c].astype(np.float64) * g
    return dict(open=open_all, yd=yd)


def signals(n, threshold_db=-30.0, seed=1):
    """[n, 2] f32 each: noise whose level wanders +-12 dB around the threshold, a train of bursts over a low floor, and a decaying tone"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    lvl = 10.0 ** ((threshold_db + 12.0 * np.sin(2 * np.pi * t / 1777.0)) / 20.0)
    noise = (rng.uniform(-1, 1, (n, 2)) * lvl[:, None] * np.sqrt(3.0)).astype(np.float32)
    burst = (rng.uniform(-1, 1, (n, 2)) * np.where((t % 700) < 90, 0.9, 0.003)[:, None]).astype(np.float32)
    env = np.exp(-(t % 9000) / 1500.0)
    tone = env * np.sin(2 * np.pi * 0.0371 * t)
    decay = np.stack([tone, 0.5 * np.roll(tone, 37)], 1).astype(np.float32)
    return {"noise": noise, "bursts": burst, "decay": decay}
