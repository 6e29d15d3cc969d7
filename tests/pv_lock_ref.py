"""ctypes binding of the CPU restatement of the locked phase vocoder (tests/pv_lock/ref_pv_lock.c), shared by
tests/test_pv_lock_cpu.py and tests/test_gpu_pv_lock.py.  Built with gcc -ffp-contract=off against oracle/libnae_oracle.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_lock", "ref_pv_lock.c")
BINS = 513


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv_lock.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.ref_pv_synth_phase.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.ref_peaks.argtypes = [C.c_void_p, C.c_void_p]
    L.ref_regions.argtypes = [C.c_void_p, C.c_void_p]
    return L


def stretch(L, x, ch, rate, pitch, lock):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = orc.plan(rate, pitch, n)
    assert rc == 0, rc
    out = np.empty(max(pl.out_len, 1) * ch, np.float32)
    assert L.ref_stretch(x.ctypes.data, n, ch, rate, pitch, int(lock), out.ctypes.data) == 0
    return out[: pl.out_len * ch]


def synth_phase(L, x, ch, rate, pitch, lock):
    """synthesis phase (Q0.32) of every frame, [frames, ch, 513] int32"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = orc.plan(rate, pitch, n)
    assert rc == 0 and pl.pv_on
    qs = np.empty((pl.frames, ch, BINS), np.int32)
    assert L.ref_pv_synth_phase(x.ctypes.data, n, ch, rate, pitch, int(lock), qs.ctypes.data) == 0
    return qs


def peaks(L, P):
    P = np.ascontiguousarray(P, np.float32)
    assert P.size == BINS
    out = np.zeros(BINS, np.uint8)
    L.ref_peaks(P.ctypes.data, out.ctypes.data)
    return out.astype(bool)


def regions(L, P):
    P = np.ascontiguousarray(P, np.float32)
    assert P.size == BINS
    out = np.zeros(BINS, np.uint16)
    L.ref_regions(P.ctypes.data, out.ctypes.data)
    return out.astype(np.int64)
