"""ctypes binding of the CPU statement of the dither (tests/dither_ref/ref_dither.c), built by tests/cstatement.py, restatements that share no
code with the C (the random source in numpy uint64, the quantiser as a plain Python loop in float64 with an exact fused step), the noise
transfer function, a Welch estimate, and the parameter sets the tests share."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dither_ref", "ref_dither.c")
MAX_TAPS, MAX_TAP_SUM, MIN_BITS, MAX_BITS = 12, 64.0, 8, 24          # NAE_DITHER_* of include/nae_dsp_spec.h
KINDS = ("none", "rectangular", "triangular", "highpass")           # NAE_DITHER_NONE ... NAE_DITHER_HIGHPASS
SHAPINGS = ("none", "first", "second", "lipshitz")                  # NAE_DITHER_SHAPE_NONE ... NAE_DITHER_SHAPE_LIPSHITZ
PRESETS = {"none": (), "first": (1.0,), "second": (2.0, -1.0), "lipshitz": (2.033, -2.165, 1.959, -1.590, 0.6149)}
G = np.uint64(0x9E3779B97F4A7C15)


class Params(C.Structure):
    """nae_dither_params of include/nae_gpu.h"""
    _fields_ = [("bits", C.c_int), ("kind", C.c_int), ("n_taps", C.c_int), ("taps", C.c_double * MAX_TAPS), ("seed", C.c_uint64)]


class State(C.Structure):
    """the statement's carried state of one stream-channel: the next sample's index, e[n - 1], e[n - 2], ..."""
    _fields_ = [("n", C.c_uint64), ("e", C.c_double * MAX_TAPS)]


def params(bits=16, kind="triangular", taps=(), seed=1):
    """taps: a preset's name or the numbers"""
    taps = PRESETS[taps] if isinstance(taps, str) else tuple(taps)
    p = Params(bits, KINDS.index(kind) if isinstance(kind, str) else kind, len(taps), (C.c_double * MAX_TAPS)(), seed)
    for k, c in enumerate(taps[:MAX_TAPS]):
        p.taps[k] = c
    return p


def taps_of(p):
    return tuple(p.taps[k] for k in range(p.n_taps))


def as_tuple(p):
    return (p.bits, p.kind, p.n_taps, tuple(p.taps), p.seed)


def drawn_taps(seed=12, count=MAX_TAPS, total=3.0):
    """`count` taps drawn uniformly and scaled to an absolute sum of `total`"""
    c = np.random.default_rng(seed).uniform(-1, 1, count)
    return tuple(float(v) for v in c * (total / np.abs(c).sum()))


# the parameter rules' table (tests/test_dither_cpu.py through the statement, tests/test_gpu_dither.py through the library): sets at the limits,
# which pass, and sets that are NAE_ERR_INVALID
BOUNDARY_PARAMS = (dict(bits=8), dict(bits=24), dict(kind=0), dict(kind=3), dict(taps=(64.0,)), dict(taps=(-32.0, 32.0)), dict(taps=(0.0,) * 12),
                   dict(taps=(5.0,) * 12), dict(seed=0), dict(seed=2 ** 64 - 1))
BAD_PARAMS = (dict(bits=7), dict(bits=25), dict(bits=0), dict(kind=-1), dict(kind=4), dict(n_taps=-1), dict(n_taps=13), dict(taps=(float("nan"),)),
              dict(taps=(1.0, float("inf"))), dict(taps=(1.0, -float("inf"))), dict(taps=(64.0, 0.001)), dict(taps=(-40.0, 30.0)), dict(taps=(5.4,) * 12))


def bad_params(changes):
    p = params(**{k: v for k, v in changes.items() if k != "n_taps"})
    if "n_taps" in changes:
        p.n_taps = changes["n_taps"]
    return p


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_dither_key.restype = C.c_uint64
    L.ref_dither_key.argtypes = [C.c_uint64] * 3
    L.ref_dither_r12.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ref_dither_d.restype = C.c_double
    L.ref_dither_d.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    L.ref_dither_check.argtypes = [C.POINTER(Params), C.c_int]
    L.ref_dither_design.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(Params)]
    L.ref_dither_run.argtypes = [C.POINTER(Params), C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(State), C.c_void_p, C.c_void_p, C.c_int]
    return L


def new_state(ch):
    return (State * ch)()


def run(L, p, x, stream=0, state=None, errors=False, after_clamp=False):
    """x[n, ch] f32 -> [n, ch] f32 as stream `stream` of a call (with errors: also e[n, ch] in double); state: new_state(ch), carried on"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    e = np.zeros(x.shape, np.float64) if errors else None
    st = new_state(x.shape[1]) if state is None else state
    assert L.ref_dither_run(C.byref(p), stream, x.ctypes.data, x.shape[0], x.shape[1], st, y.ctypes.data, e.ctypes.data if errors else None,
                            int(after_clamp)) == 0
    return (y, e) if errors else y


def run_streams(L, p, x, shared=False):
    """the statement on x[streams, n, ch]: stream s under its own key"""
    return np.stack([run(L, p, x[0 if shared else s], stream=s) for s in range(len(x))])


def in_pieces(L, p, x, cuts, stream=0):
    """x[n, ch] in pieces of the sizes in `cuts` (the last one repeated) with the state carried"""
    st, parts, pos, i = new_state(x.shape[1]), [], 0, 0
    while pos < len(x):
        k = min(cuts[min(i, len(cuts) - 1)], len(x) - pos)
        parts.append(run(L, p, x[pos:pos + k], stream, st))
        pos += k
        i += 1
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------- restatements
def fin64(z):
    """the splitmix64 finaliser on numpy uint64 (wrapping arithmetic)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key64(seed, stream, channel):
    with np.errstate(over="ignore"):
        return fin64(fin64(fin64(np.uint64(seed) + G) + np.uint64(stream)) + np.uint64(channel))


def r12(key, n):
    """r1, r2 in [-0.5, 0.5) at the sample indices n (any integer array below 2^64)"""
    with np.errstate(over="ignore"):
        h = fin64(np.uint64(key) + G * np.asarray(n, np.uint64))
    hi = (h >> np.uint64(32)).astype(np.uint32).view(np.int32)
    lo = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return hi.astype(np.float64) * 2.0 ** -32, lo.astype(np.float64) * 2.0 ** -32


def dither(kind, key, n0, count):
    """d[n0 ... n0 + count) in LSB for a kind's name"""
    n = np.arange(count, dtype=np.uint64) + np.uint64(n0)
    if kind == "none":
        return np.zeros(count)
    r1, r2 = r12(key, n)
    if kind == "rectangular":
        return r1
    if kind == "triangular":
        return r1 + r2
    with np.errstate(over="ignore"):
        before = r12(key, n - np.uint64(1))[0]
    if n0 == 0:
        before[0] = 0.0
    return r1 - before


def fma(a, b, c):
    """a b + c rounded once: exact rationals, and the conversion of a rational to float rounds correctly"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def restate(p, x, stream=0):
    """the quantiser as a plain Python loop over float64 -> (y [n, ch] f32, e [n, ch]): the specification's steps, the fused one by `fma`"""
    x = np.ascontiguousarray(x, np.float32)
    S = 2.0 ** (p.bits - 1)
    taps = taps_of(p)
    y, es = np.zeros_like(x), np.zeros(x.shape)
    for c in range(x.shape[1]):
        d = dither(KINDS[p.kind], key64(p.seed, stream, c), 0, len(x))
        e = [0.0] * len(taps)
        for n in range(len(x)):
            xi = float(x[n, c])
            u = xi * S if np.isfinite(xi) else 0.0
            for k in range(len(taps), 0, -1):
                u = fma(-taps[k - 1], e[k - 1], u)
            q = float(np.rint(u + float(d[n])))
            if taps:
                e = [q - u] + e[:-1]
            es[n, c] = q - u
            y[n, c] = np.float32(min(max(q, -S), S - 1.0) / S)
    return y, es


def ntf2(taps, omega):
    """|NTF(e^{j omega})|^2 in float64"""
    z = np.exp(-1j * np.asarray(omega, np.float64))
    h = np.ones_like(z)
    for k, c in enumerate(taps):
        h = h - c * z ** (k + 1)
    return np.abs(h) ** 2


def welch(v, seg):
    """one-sided Welch estimate with a Hann window and half-overlapping segments of `seg` samples, scaled so that white noise of variance
    s^2 reads s^2 in every bin -> (omega of the bins, the estimate, the number of segments)"""
    w = np.hanning(seg + 1)[:seg]
    starts = range(0, len(v) - seg + 1, seg // 2)
    acc = np.zeros(seg // 2 + 1)
    for s in starts:
        acc += np.abs(np.fft.rfft(v[s:s + seg] * w)) ** 2
    return np.arange(seg // 2 + 1) * (2 * np.pi / seg), acc / (len(starts) * np.sum(w ** 2)), len(starts)
