"""ctypes binding of the CPU statement of the vocoder (tests/pv_ref/ref_pv.c): every frame size, the phase lock and the formant lifter.
Built with gcc -ffp-contract=off against oracle/libnae_oracle.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_ref", "ref_pv.c")
SIZES = (512, 1024, 2048, 4096)
BINS = 513          # the peak and region rules' spectrum, N = 1024


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_pv_plan.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_synth_phase.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_peaks.argtypes = [C.c_void_p, C.c_void_p]
    L.ref_pv_regions.argtypes = [C.c_void_p, C.c_void_p]
    return L


def plan(L, rate, pitch, n_fft, n):
    pl = orc.Plan()
    rc = L.ref_pv_plan(rate, pitch, n_fft, n, C.byref(pl))
    return rc, pl


def stretch(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = plan(L, rate, pitch, n_fft, n)
    assert rc == 0, rc
    out = np.empty(max(pl.out_len, 1) * ch, np.float32)
    assert L.ref_pv_stretch(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), lifter, out.ctypes.data) == 0
    return out[: pl.out_len * ch]


def synth_phase(L, x, ch, rate, pitch, n_fft=1024, lock=False):
    """synthesis phase (Q0.32) of every frame, [frames, ch, n_fft/2 + 1] int32"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = plan(L, rate, pitch, n_fft, n)
    assert rc == 0 and pl.pv_on
    qs = np.empty((pl.frames, ch, n_fft // 2 + 1), np.int32)
    assert L.ref_pv_synth_phase(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), qs.ctypes.data) == 0
    return qs


def peaks(L, P):
    P = np.ascontiguousarray(P, np.float32)
    assert P.size == BINS
    out = np.zeros(BINS, np.uint8)
    L.ref_pv_peaks(P.ctypes.data, out.ctypes.data)
    return out.astype(bool)


def regions(L, P):
    P = np.ascontiguousarray(P, np.float32)
    assert P.size == BINS
    out = np.zeros(BINS, np.int32)
    L.ref_pv_regions(P.ctypes.data, out.ctypes.data)
    return out.astype(np.int64)


def default_lifter(sample_rate, n_fft):
    """DESIGN.md §3, "Formant preservation": min(max(sample_rate / 700, 1), n_fft / 4), integer division"""
    return min(max(sample_rate // 700, 1), n_fft // 4)
