"""The float64 numpy statement of the formant shift ("Formant shift"), on tests/pv_sizes_numpy.py: an independent
specification of what the CPU statement tests/pv_ref/ref_pv.c computes under the _formant_shift entries' rules
(tests/test_pv_fshift_cpu.py)."""
import numpy as np

import pv_sizes_numpy
from golden import pv_numpy


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
