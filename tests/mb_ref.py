"""ctypes binding of the CPU statement of the multiband compressor (tests/mb_ref/ref_mb.c), built by tests/cstatement.py, the float64
restatements of the design, of the all-pass and of the band signals, and the parameter sets the tests share.  The library holds the
statements of the equalizer and of the dynamics processor too (the file includes them), so tests/eq_ref.py's and tests/dyn_ref.py's functions
run on it."""
import ctypes as C
import math
import os

import numpy as np

import cstatement
import dyn_ref
import eq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mb_ref", "ref_mb.c")
MAX_BANDS, MAX_SECTIONS = 4, 14                        # NAE_MB_MAX_BANDS, NAE_MB_MAX_SECTIONS
CHUNK = dyn_ref.CHUNK
Q = 0.7071067811865476
SECTIONS = {2: 4, 3: 9, 4: 14}
# DESIGN.md §3, "K20 multiband": the slots of every band's path from the input on
PATHS = {2: ((0, 1), (2, 3)),
         3: ((0, 1, 2), (3, 4, 5, 6), (3, 4, 7, 8)),
         4: ((0, 1, 2, 3, 4), (0, 1, 2, 5, 6), (7, 8, 9, 10, 11), (7, 8, 9, 12, 13))}
# what stands in a slot: ("lp" | "hp" | "ap", index of the crossover)
SLOTS = {2: (("lp", 0), ("lp", 0), ("hp", 0), ("hp", 0)),
         3: (("lp", 0), ("lp", 0), ("ap", 1), ("hp", 0), ("hp", 0), ("lp", 1), ("lp", 1), ("hp", 1), ("hp", 1)),
         4: (("lp", 1), ("lp", 1), ("ap", 2), ("lp", 0), ("lp", 0), ("hp", 0), ("hp", 0), ("hp", 1), ("hp", 1), ("ap", 0), ("lp", 2), ("lp", 2),
             ("hp", 2), ("hp", 2))}
# the crossovers of the flat-sum cases, by sample rate
FLAT_CASES = ((48000, (200.0,)), (48000, (120.0, 2500.0)), (48000, (120.0, 1000.0, 6000.0)), (44100, (20.0, 40.0, 20000.0)),
              (192000, (20.0, 25.0, 90000.0)), (8000, (20.0, 1000.0, 3900.0)))


class Params(C.Structure):
    """nae_mb_params of include/nae_gpu.h"""
    _fields_ = [("n_bands", C.c_int), ("n_sections", C.c_int), ("coef", (C.c_double * 5) * MAX_SECTIONS), ("band", dyn_ref.Params * MAX_BANDS),
                ("mute_mask", C.c_uint), ("bypass_mask", C.c_uint)]


def params(coef, bands, mute_mask=0, bypass_mask=0, n_bands=None, n_sections=None):
    """coef: [n][5]; bands: tests/dyn_ref.Params each; n_bands, n_sections: counts that differ from the lengths, for the rejections"""
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    p = Params()
    p.n_bands, p.n_sections = len(bands) if n_bands is None else n_bands, coef.shape[0] if n_sections is None else n_sections
    for s, row in enumerate(coef[:MAX_SECTIONS]):
        for i, v in enumerate(row):
            p.coef[s][i] = v
    for b, band in enumerate(bands[:MAX_BANDS]):
        p.band[b] = band
    p.mute_mask, p.bypass_mask = mute_mask, bypass_mask
    return p


def coef_of(p):
    return np.array([[p.coef[s][i] for i in range(5)] for s in range(max(0, min(p.n_sections, MAX_SECTIONS)))], np.float64).reshape(-1, 5)


def bands_of(p):
    return [p.band[b] for b in range(max(0, min(p.n_bands, MAX_BANDS)))]


def with_masks(p, mute_mask=None, bypass_mask=None, bands=None):
    """a copy of p with other masks or band records"""
    return params(coef_of(p), bands_of(p) if bands is None else bands, p.mute_mask if mute_mask is None else mute_mask,
                  p.bypass_mask if bypass_mask is None else bypass_mask)


def lib_params(nae, p):
    """tests/mb_ref.Params -> the binding's MbParams"""
    return nae.MbParams.make(coef_of(p), [nae.DynParams(*dyn_ref.as_tuple(b)) for b in bands_of(p)], p.mute_mask, p.bypass_mask, p.n_bands, p.n_sections)


def path_coef(p, b):
    """the sections of band b's path, in a row"""
    return np.ascontiguousarray(coef_of(p)[list(PATHS[p.n_bands][b])])


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_mb_check.argtypes = [C.POINTER(Params), C.c_int]
    L.ref_mb_run.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_mb_bands.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_mb_split_f64.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_mb_design.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.POINTER(Params)]
    L.ref_mb_path.argtypes = [C.c_int, C.c_int, C.c_void_p]
    # the two statements it includes, under their own bindings' types
    L.ref_dyn_run.argtypes = [C.POINTER(dyn_ref.Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_dyn_design.argtypes = [C.c_int] + [C.c_double] * 7 + [C.c_int, C.POINTER(dyn_ref.Params)]
    for name in ("ref_eq_run", "ref_eq_run_f64", "ref_eq_sequential"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.ref_eq_design.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return L


def run(L, p, x):
    """x[n, ch] f32 -> [n, ch] f32: the statement"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    rc = L.ref_mb_run(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data)
    assert rc == 0, rc
    return y


def run_streams(L, p, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([run(L, p, s) for s in x])


def bands(L, p, x):
    """x[n, ch] f32 -> the band signals [n_bands, n, ch] f32 of the statement"""
    x = np.ascontiguousarray(x, np.float32)
    xb = np.zeros((p.n_bands,) + x.shape, np.float32)
    rc = L.ref_mb_bands(C.byref(p), x.ctypes.data, x.shape[0], x.shape[1], xb.ctypes.data)
    assert rc == 0, rc
    return xb


def split_f64(L, p, x, tiled=True):
    """x[n] f32 -> the band signals [n_bands, n] in double, not rounded: K11's tiled form, or the plain sequential recurrence"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    w = np.zeros((p.n_bands, x.size), np.float64)
    rc = L.ref_mb_split_f64(C.byref(p), x.ctypes.data, x.size, int(tiled), w.ctypes.data)
    assert rc == 0, rc
    return w


def design(L, sample_rate, crossovers, band_params, mute_mask=0, bypass_mask=0):
    """the statement's design (ref_mb_design): Params, or None where it refuses"""
    xs = np.ascontiguousarray(crossovers, np.float64)
    recs = (dyn_ref.Params * max(len(band_params), 1))(*band_params)
    out = Params()
    rc = L.ref_mb_design(sample_rate, len(band_params), xs.ctypes.data, C.addressof(recs), mute_mask, bypass_mask, C.byref(out))
    return out if rc == 0 else None


def allpass(sample_rate, freq, q=Q):
    """float64 restatement of the design's all-pass: the cookbook's, with the w0, alpha and q of tests/eq_ref.design, libm through `math`"""
    f = np.float64
    w0 = f(2.0) * f(math.pi) * f(freq) / f(sample_rate)
    cs, alpha = f(math.cos(w0)), f(math.sin(w0)) / (f(2.0) * f(q))
    a0 = f(1.0) + alpha
    return np.array([(f(1.0) - alpha) / a0, (f(-2.0) * cs) / a0, (f(1.0) + alpha) / a0, (f(-2.0) * cs) / a0, (f(1.0) - alpha) / a0], np.float64)


def design64(sample_rate, crossovers):
    """float64 restatement of nae_mb_design's sections: [4 | 9 | 14][5] from 1, 2 or 3 crossovers"""
    made = {"lp": [eq_ref.design("lowpass", sample_rate, f, 0.0, Q) for f in crossovers],
            "hp": [eq_ref.design("highpass", sample_rate, f, 0.0, Q) for f in crossovers],
            "ap": [allpass(sample_rate, f) for f in crossovers]}
    return np.stack([made[kind][i] for kind, i in SLOTS[len(crossovers) + 1]])


def biquads64(coef, x):
    """x[n] through the sections coef[S][5] by the plain recurrence in float64 (Python floats are IEEE doubles)"""
    v = [float(s) for s in np.asarray(x, np.float64)]
    for b0, b1, b2, a1, a2 in np.asarray(coef, np.float64).reshape(-1, 5).tolist():
        z1 = z2 = 0.0
        for n, xv in enumerate(v):
            yv = b0 * xv + z1
            z1 = (b1 * xv - a1 * yv) + z2
            z2 = b2 * xv - a2 * yv
            v[n] = yv
    return np.array(v, np.float64)


def bands64(coef, n_bands, x):
    """the float64 band signals [n_bands, n] of x[n] through the tree's paths, by the plain recurrence"""
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    return np.stack([biquads64(coef[list(path)], x) for path in PATHS[n_bands]])


def magnitude_of_sum(coef, n_bands, freq, sample_rate):
    """|sum over the bands of H_b(e^jw)| from the coefficients: 1 for a designed tree"""
    z = np.exp(-2j * np.pi * np.asarray(freq, np.float64) / sample_rate)
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    total = 0.0
    for path in PATHS[n_bands]:
        h = 1.0 + 0j
        for b0, b1, b2, a1, a2 in coef[list(path)]:
            h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
        total = total + h
    return np.abs(total)


def band_set(n_bands, lookahead=0, link=1, speed=None):
    """n_bands different compressors that all work on unit noise's bands: thresholds, slopes, knees and make-ups that differ band to band"""
    speed = dict(alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05)) if speed is None else speed
    return [dyn_ref.params(threshold_db=-36.0 + 4.0 * b, slope=(0.75, 0.5, 1.0, 0.9)[b], knee_db=(6.0, 0.0, 12.0, 3.0)[b], makeup_db=(2.0, 0.0, -1.5, 3.0)[b],
                           lookahead=lookahead, link=link, **speed) for b in range(n_bands)]


CROSSOVERS = {2: (200.0,), 3: (120.0, 2500.0), 4: (120.0, 1000.0, 6000.0)}


def case(n_bands, lookahead=0, link=1, mute_mask=0, bypass_mask=0, sample_rate=48000, speed=None):
    """the parameter set the tests share for n_bands: the designed tree at the ordinary crossovers and band_set's compressors"""
    return params(design64(sample_rate, CROSSOVERS[n_bands]), band_set(n_bands, lookahead, link, speed), mute_mask, bypass_mask)
