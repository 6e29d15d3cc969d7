"""Independent float64 restatement of the K7 node at frame size N (analysis and synthesis frames of N samples, hop
H = N/4, Hann/Hann, gain 2/3, exact Q0.32 phase accumulation; the transposer and the stage order of every size), with numpy's own FFT.
tests/golden/pv_numpy.py states the same node at N = 1024 and is kept as it is; this one takes N as a parameter and reuses its
N-independent parts (plan fields, transposer).  With a lifter q > 0 it states formant preservation ("Formant preservation"):
each synthesis frame's magnitudes multiplied by G[k] of the frame's cepstral envelope.  It pins the CPU statement tests/pv_ref/ref_pv.c to the
specification at every size."""
import numpy as np

from golden import pv_numpy


def plan(rate, pitch, L, N):
    H = N // 4
    pl = pv_numpy.plan(rate, pitch, L)
    pl["N"] = N
    pl["ha"] = int(np.floor(H * pl["tempo"] * 2 ** 24 + 0.5))
    pl["frames"] = (pl["pv_out"] + N // 2 + H - 1) // H + 1 if pl["pv_on"] else 0
    return pl


def gain(X, N, q, g):
    """G[0..N/2] of one analysis spectrum X (steps 1-5)"""
    M = N // 2
    L = np.log2(np.maximum(np.abs(X), 2.0 ** -40))
    c = np.fft.irfft(L, N)
    n = np.arange(N)
    c[~((n < q) | (n > N - q))] = 0.0
    Ls = np.fft.rfft(c).real
    u = np.float64(np.float32(np.arange(M + 1, dtype=np.float32) * np.float32(g)))
    G = np.zeros(M + 1)
    ok = u <= M
    i = np.minimum(u, M).astype(np.int64)
    t = u - i
    lu = np.where(i == M, Ls[M], Ls[np.minimum(i, M - 1)] + t * (Ls[np.minimum(i + 1, M)] - Ls[np.minimum(i, M - 1)]))
    G[ok] = np.minimum(np.exp2(lu - Ls), 16.0)[ok]
    return G


def vocoder(x, pl, M, q=0, g=1.0):
    """one channel, float64 in/out; q > 0: formant preservation with transposer ratio g"""
    N = pl["N"]
    H, bins, sh = N // 4, N // 2 + 1, 32 - int(np.log2(N))
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    k = np.arange(bins)
    v = np.zeros(M + N + H)
    d0 = pl["ha"] >> 24
    qs = qa_prev = None
    s_prev = 0
    for f in range(pl["frames"]):
        s = (((f - 1) * pl["ha"] + (1 << 23)) >> 24) - N // 2
        idx = s + np.arange(N)
        ok = (idx >= 0) & (idx < x.size)
        fr = np.where(ok, x[np.clip(idx, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
        X = np.fft.rfft(fr * w)
        qa = np.round(np.angle(X) / (2 * np.pi) * 2 ** 32).astype(np.int64) & 0xFFFFFFFF
        if f == 0:
            qs = qa.copy()
        else:
            d = s - s_prev
            R = ((H << 24) + d // 2) // d
            e = ((k * d) & (N - 1)) << sh
            dw = (qa - qa_prev - e) & 0xFFFFFFFF
            dw = np.where(dw >= 2 ** 31, dw - 2 ** 32, dw)
            adv = ((k * H) & (N - 1)) << sh
            qs = (qs + adv + ((dw * R + (1 << 23)) >> 24)) & 0xFFFFFFFF
            assert d in (d0, d0 + 1)
        qa_prev, s_prev = qa, s
        ph = np.where(qs >= 2 ** 31, qs - 2 ** 32, qs) / 2.0 ** 32 * 2 * np.pi
        mag = gain(X, N, q, g) * np.abs(X) if q > 0 else np.abs(X)
        Y = mag * np.exp(1j * ph)
        Y[0] = Y[0].real
        Y[-1] = Y[-1].real
        y = np.fft.irfft(Y, N)
        o = (f - 1) * H - N // 2
        lo, hi = max(o, 0), min(o + N, M)
        if hi > lo:
            v[lo:hi] += (w * y)[lo - o:hi - o]
    return v[:M] * (2.0 / 3.0)


def stretch(x, ch, rate, pitch, N, q=0):
    """interleaved [L*ch] -> interleaved [out_len*ch], float64; a lifter q > 0 needs both stages on (a pitch change)"""
    x = np.asarray(x, np.float64).reshape(-1, ch)
    pl = plan(rate, pitch, x.shape[0], N)
    assert q == 0 or (pl["pv_on"] and pl["rs_on"])
    g = float(np.float32(pl["rho"]))
    out = np.zeros((pl["out_len"], ch))
    tr = pv_numpy.transposer
    for c in range(ch):
        s = x[:, c]
        if not pl["pv_on"] and not pl["rs_on"]:
            out[:, c] = s
        elif pl["rs_first"]:
            out[:, c] = vocoder(tr(s, pl, pl["mid"]), pl, pl["out_len"], q, g)
        elif pl["pv_on"] and pl["rs_on"]:
            out[:, c] = tr(vocoder(s, pl, pl["mid"], q, g), pl, pl["out_len"])
        elif pl["pv_on"]:
            out[:, c] = vocoder(s, pl, pl["out_len"])
        else:
            out[:, c] = tr(s, pl, pl["out_len"])
    return out.reshape(-1)
