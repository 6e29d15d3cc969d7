"""The float64 synthesis of the vocoder from GIVEN integer synthesis phases (DESIGN.md §3, K7 and its options), in plain numpy with numpy's
own FFT: the yardstick behind the phases `Qs`.  It takes the CPU statement's Qs (pv_ref.taps) and so makes no phase-wrap decision of its own;
that makes it comparable with the statement and with the GPU at every tempo, option and stage order, where the full float64 restatements
(tests/pv_sizes_numpy.py, tests/golden/pv_numpy.py) are comparable at tempo 1/2 only.  What it restates is everything behind Qs: the
magnitudes, sin / cos, the formant gain, the inverse FFT, the window, the overlap-add, the 2/3 gain and the transposer when it runs last.
It shares no code with tests/pv_ref/ref_pv.c or the oracle beyond the plan (lengths, frame positions) and, where the transposer runs first,
the statement's bit-exact mid signal.  tests/test_pv_f64_cpu.py holds the statement to it, tests/test_gpu_pv_f64.py the kernels."""
import numpy as np

import pv_ref
from golden import pv_numpy

GAIN = 2.0 / 3.0
MAX_GAIN = 16.0                 # NAE_FORMANT_MAX_GAIN
TAPS = pv_numpy.TAPS
_tables = {}


KINDS = ("noise", "tones", "clicks")


def content(kind, n, ch, N, seed):
    """interleaved f32 [n * ch], every channel its own: white noise; two partials over noise 10 dB down (broadband, so that the envelope
    stage's log2 reads signal and not rounding noise in every bin); clicks every 2 N + 5 samples over a noise floor of 1e-3, so that
    transient preservation resets and the channel's RMS stays above 1e-3"""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.zeros((n, ch))
    for c in range(ch):
        if kind == "noise":
            x[:, c] = 0.25 * rng.standard_normal(n)
        elif kind == "tones":
            f0 = 440.0 * (1 + 0.31 * c + 0.07 * (seed % 5))
            x[:, c] = 0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * f0 * t / 48000 + c) + 0.1 * np.sin(2 * np.pi * 3.7 * f0 * t / 48000)
        else:
            x[:, c] = 1e-3 * rng.standard_normal(n)
            x[N + N // 8 + 37 * c + 11 * (seed % 7)::2 * N + 5, c] += 0.9 - 0.3 * c
    return np.ascontiguousarray(x, np.float32).reshape(-1)


def hann32(N):
    """Hann_N: double, one rounding to f32 (the tables of DESIGN.md §3), as float64 values"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32).astype(np.float64)


def rs_table(rho):
    if rho not in _tables:
        _tables[rho] = pv_numpy.rs_table(rho)
    return _tables[rho]


def transposer(v, step_q32, rho, n_out):
    """pv_numpy.transposer on whole arrays: the table rounded to f32, positions exact, everything else in double"""
    tab = rs_table(rho)
    v = np.asarray(v, np.float64)
    pos = np.arange(n_out, dtype=np.uint64) * np.uint64(step_q32)
    idx, frac = (pos >> np.uint64(32)).astype(np.int64), (pos & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ph, alpha = frac >> 25, (frac & 0x1FFFFFF) / 33554432.0
    coef = tab[ph] + alpha[:, None] * (tab[ph + 1] - tab[ph])
    m = idx[:, None] - (TAPS // 2 - 1) + np.arange(TAPS)
    ok = (m >= 0) & (m < v.size)
    taps = np.where(ok, v[np.clip(m, 0, max(v.size - 1, 0))] if v.size else 0.0, 0.0)
    return np.sum(coef * taps, axis=1)


def stage_on(rho, q, phi):
    """nae_formant_stage_on restated: the envelope stage runs with a lifter and a transposer ratio that differs from the formant ratio"""
    return q > 0 and abs(rho / phi - 1.0) >= 1e-6


def envelope(pl, lifter, formant_ratio):
    """(lifter in effect, g): the _formant entries (formant_ratio None) want both stages on and take g = (float)rate_eff; the _formant_shift
    entries want the vocoder stage (forced on by their plan where needed) and stage_on, and take g = (float)(rate_eff / phi)"""
    if formant_ratio is None:
        return (lifter if pl.pv_on and pl.rs_on else 0), float(np.float32(pl.rate_eff))
    return (lifter if pl.pv_on and stage_on(pl.rate_eff, lifter, formant_ratio) else 0), float(np.float32(pl.rate_eff / formant_ratio))


def get_plan(L, rate, pitch, n_fft, n, lifter=0, formant_ratio=None):
    rc, pl = (pv_ref.plan(L, rate, pitch, n_fft, n) if formant_ratio is None
              else pv_ref.fs_plan(L, rate, pitch, formant_ratio, lifter, n_fft, n))
    assert rc == 0, rc
    return pl


def forced(pl):
    return bool(pl.pv_on and pl.tempo_eff == 1.0)


def gains(X, N, q, g):
    """steps 1-5 of "Formant preservation" on every row of X [frames, N/2 + 1] (pv_sizes_numpy.gain, all frames at once)"""
    M = N // 2
    Lg = np.log2(np.maximum(np.abs(X), 2.0 ** -40))
    c = np.fft.irfft(Lg, N, axis=1)
    n = np.arange(N)
    c[:, ~((n < q) | (n > N - q))] = 0.0
    Ls = np.fft.rfft(c, axis=1).real
    u = (np.arange(M + 1, dtype=np.float32) * np.float32(g)).astype(np.float64)          # one f32 product, as the specification says
    ok = u <= M
    i = np.minimum(u, M).astype(np.int64)
    t = u - i
    i0, i1 = np.minimum(i, M - 1), np.minimum(i + 1, M)
    lu = np.where(i == M, Ls[:, M:M + 1], Ls[:, i0] + t * (Ls[:, i1] - Ls[:, i0]))
    return np.where(ok, np.minimum(np.exp2(lu - Ls), MAX_GAIN), 0.0)


def vocoder(x, pl, N, M, qs, q=0, g=1.0, window=None):
    """one channel: x float64 (f32 values), qs [frames, bins] int32 or None for the forced stage (Y = G X) -> float64 [M]"""
    H, bins = N // 4, N // 2 + 1
    frames = int(pl.frames)
    w = hann32(N) if window is None else window
    f = np.arange(frames, dtype=np.int64)
    s = (((f - 1) * int(pl.ha_q24) + (1 << 23)) >> 24) - N // 2
    idx = s[:, None] + np.arange(N)
    ok = (idx >= 0) & (idx < x.size)
    fr = np.where(ok, x[np.clip(idx, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
    X = np.fft.rfft(fr * w, axis=1)
    G = gains(X, N, q, g) if q > 0 else 1.0
    if qs is None:
        Y = G * X
    else:
        assert qs.shape == (frames, bins), (qs.shape, frames, bins)
        Y = G * np.abs(X) * np.exp(2j * np.pi * (qs.astype(np.float64) / 2.0 ** 32))
    Y[:, 0], Y[:, -1] = Y[:, 0].real, Y[:, -1].real
    y = np.fft.irfft(Y, N, axis=1) * w
    v = np.zeros(M + 2 * N + H)                         # frame f lands at (f - 1) H - N/2; shifted by N so that no index is negative
    for k in range(frames):                             # increasing f, as the specification adds them
        o = (k - 1) * H - N // 2 + N
        if 0 <= o and o + N <= v.size:
            v[o:o + N] += y[k]
    return v[N:N + M] * GAIN


def synth(L, x, ch, rate, pitch, n_fft, taps, lifter=0, formant_ratio=None, window=None):
    """x: interleaved f32 [n * ch]; taps: the statement's Qs [frames, ch, bins] int32 (pv_ref.taps(...)[0] of the same call; locked, transient
    and linked runs differ in these integers alone), None where the plan has no vocoder stage or a forced one -> float64 [out_len * ch].
    L is the built statement (pv_ref.build): it gives the plan and, where the transposer runs first, its bit-exact output."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // ch
    pl = get_plan(L, rate, pitch, n_fft, n, lifter, formant_ratio)
    xc = x.reshape(n, ch).astype(np.float64)
    if not pl.pv_on and not pl.rs_on:
        return xc.reshape(-1)
    if not pl.pv_on:
        return np.stack([transposer(xc[:, c], pl.step_q32, pl.rate_eff, pl.out_len) for c in range(ch)], 1).reshape(-1)
    q, g = envelope(pl, lifter, formant_ratio)
    if forced(pl):
        assert q > 0 and taps is None
    else:
        assert taps is not None and taps.shape[0] == pl.frames and taps.shape[1] == ch, (None if taps is None else taps.shape, pl.frames)
    if pl.rs_first:
        mid = pv_ref.stretch(L, x, ch, pl.rate_eff, 1.0)                   # specified bit for bit: the statement's own mid signal
        assert mid.size == pl.mid_len * ch, (mid.size, pl.mid_len)
        xc = mid.reshape(pl.mid_len, ch).astype(np.float64)
    M = pl.out_len if pl.rs_first else pl.mid_len
    out = np.zeros((pl.out_len, ch))
    for c in range(ch):
        v = vocoder(xc[:, c], pl, n_fft, M, None if taps is None else taps[:, c], q, g, window)
        out[:, c] = transposer(v, pl.step_q32, pl.rate_eff, pl.out_len) if pl.rs_on and not pl.rs_first else v
    return out.reshape(-1)


def measures(y, r, hop):
    """one stream-channel: y against the float64 r -> (e_rms, e_blk, e_max), each divided by sigma = RMS of r:
    the whole signal's RMS error, the largest RMS error over blocks of `hop` samples aligned to sample 0 (the ragged last block counts as
    a whole block whose missing samples have no error, so that a handful of samples is not read as a block), and the largest error"""
    y, r = np.asarray(y, np.float64), np.asarray(r, np.float64)
    assert y.shape == r.shape and y.ndim == 1 and y.size, (y.shape, r.shape)
    sigma = float(np.sqrt(np.mean(r * r)))
    assert sigma >= 1e-3, sigma
    d2 = (y - r) ** 2
    pad = (-d2.size) % hop
    blk = np.concatenate([d2, np.zeros(pad)]).reshape(-1, hop).mean(axis=1)
    return float(np.sqrt(d2.mean())) / sigma, float(np.sqrt(blk.max())) / sigma, float(np.sqrt(d2.max())) / sigma


def channel_measures(y, r, ch, hop):
    """measures() of every channel of the interleaved y, r -> [ch] tuples"""
    y, r = np.asarray(y).reshape(-1, ch), np.asarray(r).reshape(-1, ch)
    return [measures(y[:, c], r[:, c], hop) for c in range(ch)]
