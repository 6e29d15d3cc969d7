"""ctypes binding of the CPU statement of the keyed dynamics (tests/dynkey_ref/ref_dynkey.c), built by tests/cstatement.py.  The library holds
the statements of the equalizer and of the dynamics processor too (the file includes them), so tests/eq_ref.py's and tests/dyn_ref.py's
functions run on it."""
import ctypes as C
import os

import numpy as np

import cstatement
import dyn_ref
import eq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dynkey_ref", "ref_dynkey.c")
MAX_SECTIONS = 4                                       # NAE_DYNKEY_MAX_SECTIONS
CHUNK = dyn_ref.CHUNK


class Params(C.Structure):
    """nae_dynkey_params of include/nae_gpu.h"""
    _fields_ = [("dyn", dyn_ref.Params), ("key_ch", C.c_int), ("n_sections", C.c_int), ("coef", (C.c_double * 5) * MAX_SECTIONS)]


def params(dyn, key_ch=0, coef=(), n_sections=None):
    """dyn: tests/dyn_ref.Params; coef: [n][5]; n_sections: a count that differs from len(coef), for the rejections"""
    coef = np.asarray(coef, np.float64).reshape(-1, 5)
    p = Params()
    p.dyn = dyn
    p.key_ch, p.n_sections = key_ch, coef.shape[0] if n_sections is None else n_sections
    for s, row in enumerate(coef[:MAX_SECTIONS]):
        for i, v in enumerate(row):
            p.coef[s][i] = v
    return p


def coef_of(p):
    return np.array([[p.coef[s][i] for i in range(5)] for s in range(max(0, min(p.n_sections, MAX_SECTIONS)))], np.float64).reshape(-1, 5)


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_dynkey_check.argtypes = [C.POINTER(Params), C.c_int]
    for name in ("ref_dynkey_run", "ref_dynkey_run_f64", "ref_dynkey_sequential", "ref_dynkey_magnitude"):
        getattr(L, name).argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    # the two statements it includes, under their own bindings' types
    L.ref_dyn_run.argtypes = [C.POINTER(dyn_ref.Params), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.ref_eq_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    return L


def _call(fn, p, x, key, out_dtype, out_ch=None):
    x = np.ascontiguousarray(x, np.float32)
    key = None if key is None else np.ascontiguousarray(key, np.float32)
    assert (key is None) == (p.key_ch == 0) and (key is None or key.shape == (x.shape[0], p.key_ch))
    out = np.zeros((x.shape[0], out_ch or x.shape[1]), out_dtype)
    rc = fn(C.byref(p), x.ctypes.data, None if key is None else key.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data)
    assert rc == 0, rc
    return out


def run(L, p, x, key=None):
    """x[n, ch] f32, key[n, key_ch] f32 or None -> [n, ch] f32: the tiled statement"""
    return _call(L.ref_dynkey_run, p, x, key, np.float32)


def run_f64(L, p, x, key=None):
    """the tiled statement in front of its final rounding"""
    return _call(L.ref_dynkey_run_f64, p, x, key, np.float64)


def sequential(L, p, x, key=None):
    """the plain sequential recurrences, not rounded"""
    return _call(L.ref_dynkey_sequential, p, x, key, np.float64)


def magnitude(L, p, x, key=None):
    """m[n, key channels] f32 of the tiled statement"""
    return _call(L.ref_dynkey_magnitude, p, x, key, np.float32, p.key_ch or np.asarray(x).shape[1])


def run_streams(L, p, x, key=None):
    """the statement on x[streams, n, ch] with key[streams or 1, n, key_ch] (one key for every stream) or None"""
    return np.stack([run(L, p, s, None if key is None else key[min(i, len(key) - 1)]) for i, s in enumerate(x)])


def eq_f32(L, coef, key):
    """key[n, kc] through the equalizer's tiled statement -> [n, kc] f32: what nae_eq_block_f32 makes of it"""
    key = np.ascontiguousarray(key, np.float32)
    return eq_ref.run(L, coef, key.reshape(-1), ch=key.shape[1]).reshape(key.shape)


def key_filters(sample_rate=48000):
    """the key filters the tests share, by section count: none, a high-pass, and four slow sections (low shelves at 30 Hz, Q 0.3, whose
    responses last many chunks: the carry between chunks and launches decides the bits)"""
    return {0: np.zeros((0, 5)), 1: eq_ref.design("highpass", sample_rate, 150.0, 0.0, 0.7071).reshape(1, 5),
            4: np.stack([eq_ref.design("lowshelf", sample_rate, 30.0, g, 0.3) for g in (6.0, -4.0, 5.0, -3.0)])}
