"""ctypes binding of the CPU restatement of the vocoder at every frame size (tests/pv_sizes/ref_pv_sizes.c), shared by
tests/test_pv_sizes_cpu.py and tests/test_gpu_pv_sizes.py.  Built with gcc -ffp-contract=off against oracle/libnae_oracle.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_sizes", "ref_pv_sizes.c")
SIZES = (512, 1024, 2048, 4096)


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv_sizes.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_plan_n.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_stretch_n.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.ref_pv_synth_phase_n.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    return L


def plan(L, rate, pitch, n_fft, n):
    pl = orc.Plan()
    rc = L.ref_plan_n(rate, pitch, n_fft, n, C.byref(pl))
    return rc, pl


def stretch(L, x, ch, rate, pitch, n_fft):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = plan(L, rate, pitch, n_fft, n)
    assert rc == 0, rc
    out = np.empty(max(pl.out_len, 1) * ch, np.float32)
    assert L.ref_stretch_n(x.ctypes.data, n, ch, rate, pitch, n_fft, out.ctypes.data) == 0
    return out[: pl.out_len * ch]


def synth_phase(L, x, ch, rate, pitch, n_fft):
    """synthesis phase (Q0.32) of every frame, [frames, ch, n_fft/2 + 1] int32"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = plan(L, rate, pitch, n_fft, n)
    assert rc == 0 and pl.pv_on
    qs = np.empty((pl.frames, ch, n_fft // 2 + 1), np.int32)
    assert L.ref_pv_synth_phase_n(x.ctypes.data, n, ch, rate, pitch, n_fft, qs.ctypes.data) == 0
    return qs
