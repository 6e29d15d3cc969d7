"""The float64 truths and the local measures of the three feed-forward filters (DESIGN.md §3, K9 FIR filter, K10 long convolution,
K18 saturation), in plain numpy: the yardstick behind tests/test_lin_f64_cpu.py (the CPU statements) and tests/test_gpu_lin_f64.py (the
kernels).  It has no C code and takes nothing from the statements but their outputs: the truth of K9 and K10 is the causal float64
convolution (fir_ref.direct, conv_ref.direct), the truth of K18 is sat_ref.run_np.

A whole-signal relative RMS cannot see anything local: a wrong block edge, a dropped last partition, a tile's halo or one tap row vanish in
it.  So every stream-channel gets three measures (e_rms, e_blk, e_max): the whole signal's relative RMS error as before, the largest RMS
error of a block and the largest error of a sample, the last two divided by a scale that is computed in float64 from the inputs alone:
  * K9, K10: blocks of B = n_fft / 2 samples aligned to sample 0 and the block scale S_b of block_scale(): the level block b would have
    for a white input at the local level of the segments that feed it.  Behind a level step, in a stop band and in the tail of a burst it
    follows the signal down, so the f32 noise of a block is measured against what that block was computed from.  Where S_b is exactly 0
    nothing feeds the block and the output must be exactly 0 (of either sign): asserted, not measured.
  * K18: blocks of 64 samples and the channel's sigma, the RMS of the float64 result, for all three (a shaped signal has no quiet blocks).
The measured values and the caps: profiles/r29_lin_f64.md."""
import numpy as np

import conv_ref
import fir_ref

KINDS = ("noise", "step", "burst", "tones")
SAT_BLOCK = 64
# (e_rms, e_blk, e_max) per node, and (e_rms, e_max) of the M = 1 map: 4 times the largest value the CPU statement reaches over the matrix of
# tests/test_lin_f64_cpu.py, rounded up to one significant digit.  The largest values: profiles/r29_lin_f64.md
CAPS = {"K9": (2e-5, 9e-7, 2e-5), "K10": (3e-6, 2e-6, 4e-6), "K18": (2e-6, 2e-6, 9e-6), "K18 map": (2e-7, 9e-7)}


def content(kind, n, ch, B, seed, amp=1.0):
    """x[n, ch] f32, every channel its own: `noise` uniform in +-amp, flat; `step` that noise with its level 60 dB down from sample
    4 B + 37 to 8 B - 11 (four blocks, the edges off the block boundaries); `burst` B samples of it from sample 5 on and silence to the end;
    `tones` the two partials of tests/test_fir_cpu.py, detuned per channel and seed"""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.zeros((n, ch))
    for c in range(ch):
        if kind == "tones":
            k = 1.0 + 0.013 * c + 0.003 * (seed % 5)
            x[:, c] = amp * (0.6 * np.sin(2 * np.pi * 0.0371 * k * t + c) + 0.3 * np.sin(2 * np.pi * 0.213 * k * t + 1.0))
            continue
        v = amp * rng.uniform(-1, 1, n)
        if kind == "step":
            v[4 * B + 37:8 * B - 11] *= 1e-3
        elif kind == "burst":
            v[:5] = 0.0
            v[5 + B:] = 0.0
        x[:, c] = v
    return np.ascontiguousarray(x, np.float32)


TAP_KINDS = ("uniform", "lowpass", "highpass", "decay")


def taps(kind, L, seed, db=100.0):
    """[L] f32: `uniform` in +-1; `lowpass` 1 kHz and `highpass` 8 kHz at 48 kHz from fir_ref.design, rounded once (L odd); `decay` uniform
    taps under an exponential that falls by `db` dB from the first tap to the last"""
    assert kind in TAP_KINDS, kind
    if kind == "lowpass":
        return fir_ref.design("lowpass", 48000, 0.0, 1000.0, L).astype(np.float32)
    if kind == "highpass":
        return fir_ref.design("highpass", 48000, 8000.0, 0.0, L).astype(np.float32)
    h = np.random.default_rng(seed).uniform(-1, 1, L)
    if kind == "decay":
        h *= 10.0 ** (-db / 20.0 * np.arange(L) / max(L - 1, 1))
    return h.astype(np.float32)


def truth(h, x, long=False):
    """x[n, ch] (f32 values) -> float64 [n, ch]: the causal convolution of every channel with h[L], or of channel c with h[c] of h[ch, L];
    long: by conv_ref.direct (FFT in double) instead of fir_ref.direct (the direct sum)"""
    h, x = np.asarray(h), np.asarray(x)
    fn = conv_ref.direct if long else fir_ref.direct
    return np.stack([fn(h if h.ndim == 1 else h[c], x[:, c]) for c in range(x.shape[1])], 1)


def block_scale(h, x, B):
    """one channel: S_b of every block of B samples of the output (the last one may be ragged), float64 [blocks].  E_h(p) the sum of squares of
    the taps of partition p (taps p B ... p B + B - 1), E_x(k) that of input block k (0 for k < 0):
        S_b^2 = sum_p E_h(p) (E_x(b - p) + E_x(b - p - 1)) / B
    partition p reaches block b from the input blocks b - p and b - p - 1 alone, so S_b = 0 exactly where every tap that could reach the
    block is 0 or meets silence"""
    h, x = np.asarray(h, np.float64), np.asarray(x, np.float64)
    assert h.ndim == x.ndim == 1 and h.size and x.size
    nb = -(-x.size // B)
    e_h = np.concatenate([h * h, np.zeros((-h.size) % B)]).reshape(-1, B).sum(axis=1)
    e_x = np.concatenate([x * x, np.zeros(nb * B - x.size)]).reshape(nb, B).sum(axis=1)
    pair = e_x + np.concatenate([[0.0], e_x[:-1]])
    return np.sqrt(np.convolve(e_h, pair)[:nb] / B)             # sums of non-negative products: 0 only where every term is 0


def measures(y, r, scale, B):
    """one stream-channel of K9 or K10: y against the float64 r with the block scales `scale` -> (e_rms, e_blk, e_max, blocks of scale 0).
    e_rms divides the whole signal's RMS error by r's RMS; e_blk is the largest RMS error of a block over its S_b (the ragged last block
    is divided by B like a whole one, on both sides), e_max the largest |error| of a sample over the S_b of its block.  In a block of scale 0
    every sample of y must be a zero."""
    y, r = np.asarray(y, np.float64), np.asarray(r, np.float64)
    assert y.shape == r.shape and y.ndim == 1 and y.size and scale.shape == (-(-y.size // B),), (y.shape, r.shape, scale.shape)
    pad = scale.size * B - y.size
    d = np.concatenate([y - r, np.zeros(pad)]).reshape(-1, B)
    silent = scale == 0.0
    if silent.any():
        out = np.concatenate([y, np.zeros(pad)]).reshape(-1, B)[silent]
        assert not out.any(), f"{int(np.count_nonzero(out))} samples are not 0 in blocks that nothing feeds: {np.flatnonzero(silent)[out.any(axis=1)][:8]}"
    live = ~silent
    assert live.any() and np.any(r), "nothing to measure"
    s = scale[live]
    e_rms = float(np.sqrt(np.sum(d * d) / np.sum(r * r)))
    e_blk = float(np.max(np.sqrt(np.mean(d[live] ** 2, axis=1)) / s))
    e_max = float(np.max(np.max(np.abs(d[live]), axis=1) / s))
    return e_rms, e_blk, e_max, int(silent.sum())


def channel_measures(y, r, h, x, B):
    """measures() of every channel of y[n, ch] against r[n, ch], the scales from h ([L] or [ch, L]) and x[n, ch] -> [ch] tuples"""
    h = np.asarray(h)
    return [measures(y[:, c], r[:, c], block_scale(h if h.ndim == 1 else h[c], x[:, c], B), B) for c in range(y.shape[1])]


def sat_measures(y, r, block=SAT_BLOCK):
    """one stream-channel of K18: (e_rms, e_blk, e_max), each divided by sigma = the RMS of the float64 r: the whole signal's RMS error, the
    largest RMS error of a block of 64 samples aligned to sample 0 (the ragged last one divided by 64 like a whole one), the largest error"""
    y, r = np.asarray(y, np.float64), np.asarray(r, np.float64)
    assert y.shape == r.shape and y.ndim == 1 and y.size, (y.shape, r.shape)
    sigma = float(np.sqrt(np.mean(r * r)))
    assert sigma > 0.0
    d2 = (y - r) ** 2
    blk = np.concatenate([d2, np.zeros((-d2.size) % block)]).reshape(-1, block).mean(axis=1)
    return float(np.sqrt(d2.mean())) / sigma, float(np.sqrt(blk.max())) / sigma, float(np.sqrt(d2.max())) / sigma


def sat_channel_measures(y, r):
    return [sat_measures(y[:, c], r[:, c]) for c in range(y.shape[1])]
