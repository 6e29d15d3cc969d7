"""ctypes binding of the CPU statement of the vocoder with transient preservation (tests/pv_transient/ref_pv_tr.c, which includes
tests/pv_ref/ref_pv.c).  Built with gcc -ffp-contract=off against oracle/libnae_oracle.so, like tests/pv_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc
import pv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_transient", "ref_pv_tr.c")


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv_tr.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_pv_plan.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_synth_phase.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_tr_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p]
    L.ref_pv_tr_synth_phase.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_tr_onsets.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.ref_pv_tr_onset_rule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def stretch(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, transients=True):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = pv_ref.plan(L, rate, pitch, n_fft, n)
    assert rc == 0, rc
    out = np.empty(max(pl.out_len, 1) * ch, np.float32)
    assert L.ref_pv_tr_stretch(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), lifter, int(transients), out.ctypes.data) == 0
    return out[: pl.out_len * ch]


def synth_phase(L, x, ch, rate, pitch, n_fft=1024, lock=False, transients=True):
    """synthesis phase (Q0.32) of every frame, [frames, ch, n_fft/2 + 1] int32"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = pv_ref.plan(L, rate, pitch, n_fft, n)
    assert rc == 0 and pl.pv_on
    qs = np.empty((pl.frames, ch, n_fft // 2 + 1), np.int32)
    assert L.ref_pv_tr_synth_phase(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), int(transients), qs.ctypes.data) == 0
    return qs


def onsets(L, x, ch, rate, pitch, n_fft=1024):
    """the onset verdict of every frame, [frames, ch] bool"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = pv_ref.plan(L, rate, pitch, n_fft, n)
    assert rc == 0 and pl.pv_on
    on = np.zeros((pl.frames, ch), np.uint8)
    assert L.ref_pv_tr_onsets(x.ctypes.data, n, ch, rate, pitch, n_fft, on.ctypes.data) == 0
    return on.astype(bool)


def onset_rule(L, P, n_fft):
    """the rule of DESIGN.md §3 on power spectra P[frames, bins] (float32) of frame size n_fft -> [frames] bool"""
    P = np.ascontiguousarray(P, np.float32)
    frames, bins = P.shape
    on = np.zeros(frames, np.uint8)
    L.ref_pv_tr_onset_rule(P.ctypes.data, frames, bins, n_fft, on.ctypes.data)
    return on.astype(bool)
