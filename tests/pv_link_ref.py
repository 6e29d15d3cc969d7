"""ctypes binding of the CPU statement of the vocoder with the channel link (tests/pv_link/ref_pv_link.c, which includes
tests/pv_fshift/ref_pv_fs.c, tests/pv_transient/ref_pv_tr.c and tests/pv_ref/ref_pv.c).  Built with gcc -ffp-contract=off against
oracle/libnae_oracle.so, like tests/pv_tr_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc
import pv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_link", "ref_pv_link.c")


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv_link.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_pv_plan.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_fs_plan.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_tr_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p]
    L.ref_pv_tr_synth_phase.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_fs_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_double, C.c_void_p]
    L.ref_pv_link_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_double, C.c_int, C.c_void_p]
    L.ref_pv_link_taps.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    return L


def _plan(L, rate, pitch, n_fft, n, lifter=0, formant_ratio=None):
    if formant_ratio is None:
        return pv_ref.plan(L, rate, pitch, n_fft, n)
    pl = orc.Plan()
    rc = L.ref_pv_fs_plan(rate, pitch, formant_ratio, lifter, n_fft, n, C.byref(pl))
    return rc, pl


def stretch_rc(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, transients=False, link=True, formant_ratio=None):
    """(return code, interleaved [out_len*ch] or None); formant_ratio given: the _formant_shift entries' rules"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = _plan(L, rate, pitch, n_fft, n, lifter, formant_ratio)
    out = np.empty(max(pl.out_len if rc == 0 else 0, 1) * ch, np.float32)
    rc = L.ref_pv_link_stretch(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), lifter, int(transients), int(formant_ratio is not None),
                               1.0 if formant_ratio is None else formant_ratio, int(link), out.ctypes.data)
    return rc, (out[: pl.out_len * ch] if rc == 0 else None)


def stretch(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, transients=False, link=True, formant_ratio=None):
    rc, y = stretch_rc(L, x, ch, rate, pitch, n_fft, lock, lifter, transients, link, formant_ratio)
    assert rc == 0, rc
    return y


def taps(L, x, ch, rate, pitch, n_fft=1024, lock=False, transients=False, link=True):
    """per frame and channel: Qs [frames, ch, bins] int32, the onset verdict the channel acts on [frames, ch] bool, and sigma
    [frames, ch, bins] int32 (locked; the identity where no map is taken)"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = pv_ref.plan(L, rate, pitch, n_fft, n)
    assert rc == 0 and pl.pv_on
    bins = n_fft // 2 + 1
    qs = np.empty((pl.frames, ch, bins), np.int32)
    on = np.zeros((pl.frames, ch), np.uint8)
    sig = np.empty((pl.frames, ch, bins), np.int32)
    assert L.ref_pv_link_taps(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), int(transients), int(link), qs.ctypes.data, on.ctypes.data,
                              sig.ctypes.data) == 0
    return qs, on.astype(bool), sig


def synth_phase(L, x, ch, rate, pitch, n_fft=1024, lock=False, transients=False, link=True):
    return taps(L, x, ch, rate, pitch, n_fft, lock, transients, link)[0]
