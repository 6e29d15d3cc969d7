"""The formant shift's two statements ("Formant shift"): the ctypes binding of the CPU statement tests/pv_fshift/ref_pv_fs.c
(which includes tests/pv_transient/ref_pv_tr.c and tests/pv_ref/ref_pv.c; built with gcc -ffp-contract=off against oracle/libnae_oracle.so,
like tests/pv_tr_ref.py), and an independent float64 numpy statement on tests/pv_sizes_numpy.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc
import pv_sizes_numpy
from golden import pv_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_fshift", "ref_pv_fs.c")
SHIFT_MIN, SHIFT_MAX = 0.25, 4.0


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    so = os.path.join(out_dir, "libref_pv_fs.so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", SRC, "-o", so,
                        "-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_pv_plan.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_tr_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p]
    L.ref_pv_fs_plan.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_fs_stretch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                    C.c_void_p]
    L.ref_pv_fs_forced_phase_diff.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_double]
    L.ref_pv_fs_forced_phase_diff.restype = C.c_longlong
    return L


def plan(L, rate, pitch, phi, lifter, n_fft, n):
    pl = orc.Plan()
    rc = L.ref_pv_fs_plan(rate, pitch, phi, lifter, n_fft, n, C.byref(pl))
    return rc, pl


def stretch(L, x, ch, rate, pitch, phi, n_fft=1024, lock=False, lifter=0, transients=False):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    rc, pl = plan(L, rate, pitch, phi, lifter, n_fft, n)
    assert rc == 0, rc
    out = np.empty(max(pl.out_len, 1) * ch, np.float32)
    assert L.ref_pv_fs_stretch(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), lifter, int(transients), phi, out.ctypes.data) == 0
    return out[: pl.out_len * ch]


def forced_phase_diff(L, x, ch, rate, pitch, phi, n_fft, lock, lifter, transients):
    """the (frame, bin) pairs of the vocoder stage with Qs != Qa"""
    x = np.ascontiguousarray(x, np.float32)
    return int(L.ref_pv_fs_forced_phase_diff(x.ctypes.data, x.size // ch, ch, rate, pitch, n_fft, int(lock), lifter, int(transients), phi))


def plan_fields(pl):
    return (pl.pv_on, pl.rs_on, pl.tempo_eff, pl.rate_eff, pl.ha_q24, pl.d0, tuple(pl.r_q24), pl.step_q32, pl.out_len, pl.mid_len, pl.frames,
            pl.rs_first)


# ---------------------------------------------------------------------------------------------------- the float64 statement
def stage_on(rho, q, phi):
    return q > 0 and abs(rho / phi - 1.0) >= 1e-6


def numpy_plan(rate, pitch, L, N, q, phi):
    """pv_sizes_numpy.plan, with the vocoder stage forced on at tempo 1 where the envelope stage runs without a tempo change"""
    pl = pv_sizes_numpy.plan(rate, pitch, L, N)
    pl["forced"] = False
    if not pl["pv_on"] and stage_on(pl["rho"], q, phi):
        H = N // 4
        pl["pv_on"], pl["forced"] = True, True
        pl["rs_first"] = bool(pl["rs_on"] and pl["rho"] > 1.0)
        pl["ha"] = H << 24
        if pl["rs_first"]:
            pl["mid"] = int(np.floor(L / pl["rho"] + 0.5))
        pl["pv_out"] = pl["out_len"] if pl["rs_first"] else pl["mid"]
        pl["frames"] = (pl["pv_out"] + N // 2 + H - 1) // H + 1
    return pl


def stft_stage(x, N, M, q, g):
    """the forced stage in float64: frame f at (f - 1) H - N/2, Y = G X, Hann, overlap-add, gain 2/3 — no phases at all"""
    H = N // 4
    frames = (M + N // 2 + H - 1) // H + 1
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    v = np.zeros(M + N + H)
    for f in range(frames):
        s = (f - 1) * H - N // 2
        idx = s + np.arange(N)
        ok = (idx >= 0) & (idx < x.size)
        fr = np.where(ok, x[np.clip(idx, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
        X = np.fft.rfft(fr * w)
        Y = pv_sizes_numpy.gain(X, N, q, g) * X
        Y[0], Y[-1] = Y[0].real, Y[-1].real
        y = np.fft.irfft(Y, N)
        lo, hi = max(s, 0), min(s + N, M)
        if hi > lo:
            v[lo:hi] += (w * y)[lo - s:hi - s]
    return v[:M] * (2.0 / 3.0)


def numpy_stretch(x, ch, rate, pitch, N, q, phi):
    """interleaved [L*ch] -> interleaved [out_len*ch], float64"""
    x = np.asarray(x, np.float64).reshape(-1, ch)
    pl = numpy_plan(rate, pitch, x.shape[0], N, q, phi)
    if not (pl["pv_on"] and stage_on(pl["rho"], q, phi)):
        q = 0
    g = float(np.float32(pl["rho"] / phi))
    out = np.zeros((pl["out_len"], ch))
    tr = pv_numpy.transposer
    voc = (lambda s, M: stft_stage(s, N, M, q, g)) if pl["forced"] else (lambda s, M: pv_sizes_numpy.vocoder(s, pl, M, q, g))
    for c in range(ch):
        s = x[:, c]
        if not pl["pv_on"] and not pl["rs_on"]:
            out[:, c] = s
        elif pl["rs_first"]:
            out[:, c] = voc(tr(s, pl, pl["mid"]), pl["out_len"])
        elif pl["pv_on"] and pl["rs_on"]:
            out[:, c] = tr(voc(s, pl["mid"]), pl, pl["out_len"])
        elif pl["pv_on"]:
            out[:, c] = voc(s, pl["out_len"])
        else:
            out[:, c] = tr(s, pl, pl["out_len"])
    return out.reshape(-1)
