"""ctypes binding of the CPU statement of the vocoder (tests/pv_ref/ref_pv.c): every frame size, the phase lock, the formant lifter,
transient preservation, the formant shift and the channel link.  Built by tests/cstatement.py against oracle/libnae_oracle.so."""
import ctypes as C
import os

import numpy as np

import cstatement
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pv_ref", "ref_pv.c")
SIZES = (512, 1024, 2048, 4096)
BINS = 513          # the peak and region rules' spectrum, N = 1024
SHIFT_MIN, SHIFT_MAX = 0.25, 4.0


def build(out_dir):
    orc.lib()                                           # builds oracle/libnae_oracle.so when it is missing
    L = cstatement.build(SRC, out_dir, ("-L" + orc.ORACLE_DIR, "-lnae_oracle", "-Wl,-rpath," + orc.ORACLE_DIR))
    L.ref_pv_plan.argtypes = [C.c_double, C.c_double, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    L.ref_pv_fs_plan.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_size_t, C.POINTER(orc.Plan)]
    # src, L, ch, rate, pitch, N, lock, q, transients, shift, phi, link, dst, qs, on, sig, qdiff
    L.ref_pv_run.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    L.ref_pv_onset_rule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ref_pv_peaks.argtypes = [C.c_void_p, C.c_void_p]
    L.ref_pv_regions.argtypes = [C.c_void_p, C.c_void_p]
    return L


def plan(L, rate, pitch, n_fft, n):
    pl = orc.Plan()
    rc = L.ref_pv_plan(rate, pitch, n_fft, n, C.byref(pl))
    return rc, pl


def fs_plan(L, rate, pitch, phi, lifter, n_fft, n):
    """the plan of the _formant_shift entries"""
    pl = orc.Plan()
    rc = L.ref_pv_fs_plan(rate, pitch, phi, lifter, n_fft, n, C.byref(pl))
    return rc, pl


def plan_fields(pl):
    return (pl.pv_on, pl.rs_on, pl.tempo_eff, pl.rate_eff, pl.ha_q24, pl.d0, tuple(pl.r_q24), pl.step_q32, pl.out_len, pl.mid_len, pl.frames,
            pl.rs_first)


def _run(L, x, ch, rate, pitch, n_fft, lock, lifter, transients, formant_ratio, link, want_out=False, want_taps=False, want_qdiff=False):
    """(return code, plan, out, (qs, on, sig), qdiff); formant_ratio given: the _formant_shift entries' rules"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    shift = formant_ratio is not None
    rc, pl = fs_plan(L, rate, pitch, formant_ratio, lifter, n_fft, n) if shift else plan(L, rate, pitch, n_fft, n)
    out = np.empty(max(pl.out_len if rc == 0 else 0, 1) * ch, np.float32) if want_out else None
    frames, bins = (pl.frames if rc == 0 and pl.pv_on else 0), n_fft // 2 + 1
    qs, on, sig = ((np.empty((frames, ch, bins), np.int32), np.zeros((frames, ch), np.uint8), np.empty((frames, ch, bins), np.int32))
                   if want_taps else (None, None, None))
    qdiff = C.c_longlong(0)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = L.ref_pv_run(x.ctypes.data, n, ch, rate, pitch, n_fft, int(lock), lifter, int(transients), int(shift), formant_ratio if shift else 1.0,
                      int(link), ptr(out), ptr(qs), ptr(on), ptr(sig), C.byref(qdiff) if want_qdiff else None)
    return rc, pl, out, (qs, on, sig), qdiff.value


def stretch_rc(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, transients=False, formant_ratio=None, link=False):
    """(return code, interleaved [out_len*ch] or None); formant_ratio given: the _formant_shift entries' rules"""
    rc, pl, out, _, _ = _run(L, x, ch, rate, pitch, n_fft, lock, lifter, transients, formant_ratio, link, want_out=True)
    return rc, (out[: pl.out_len * ch] if rc == 0 else None)


def stretch(L, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, transients=False, formant_ratio=None, link=False):
    """x: interleaved [n*ch] f32 -> interleaved [out_len*ch]"""
    rc, y = stretch_rc(L, x, ch, rate, pitch, n_fft, lock, lifter, transients, formant_ratio, link)
    assert rc == 0, rc
    return y


def taps(L, x, ch, rate, pitch, n_fft=1024, lock=False, transients=False, link=False):
    """per frame and channel: Qs (Q0.32) [frames, ch, bins] int32, the onset verdict the channel acts on [frames, ch] bool (whatever
    `transients` says), and sigma [frames, ch, bins] int32 (locked; the identity where no map is taken)"""
    rc, pl, _, (qs, on, sig), _ = _run(L, x, ch, rate, pitch, n_fft, lock, 0, transients, None, link, want_taps=True)
    assert rc == 0 and pl.pv_on, rc
    return qs, on.astype(bool), sig


def synth_phase(L, x, ch, rate, pitch, n_fft=1024, lock=False, transients=False, link=False):
    """synthesis phase (Q0.32) of every frame, [frames, ch, n_fft/2 + 1] int32"""
    return taps(L, x, ch, rate, pitch, n_fft, lock, transients, link)[0]


def onsets(L, x, ch, rate, pitch, n_fft=1024):
    """the onset verdict of every frame, [frames, ch] bool; unlinked, it depends on neither the lock nor the flag"""
    return taps(L, x, ch, rate, pitch, n_fft)[1]


def onset_rule(L, P, n_fft):
    """the rule of DESIGN.md §3 on power spectra P[frames, bins] (float32) of frame size n_fft -> [frames] bool"""
    P = np.ascontiguousarray(P, np.float32)
    frames, bins = P.shape
    on = np.zeros(frames, np.uint8)
    L.ref_pv_onset_rule(P.ctypes.data, frames, bins, n_fft, on.ctypes.data)
    return on.astype(bool)


def forced_phase_diff(L, x, ch, rate, pitch, phi, n_fft, lock, lifter, transients):
    """the (frame, channel, bin) triples of the vocoder stage with Qs != Qa under the _formant_shift entries' rules; -1 without the stage"""
    rc, _, _, _, n = _run(L, x, ch, rate, pitch, n_fft, lock, lifter, transients, phi, False, want_qdiff=True)
    return -1 if rc else n


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
