#!/usr/bin/env python3
"""Randomised differential run (GPU box) over the whole supported K7 range: frame sizes 512 ... 4096 (the phase lock at 1024), log-uniform
tempo over [1/64, 16] and transposer ratio over [1/16, 16], edge-heavy input lengths, batches around the size-generic tile policy's switch
(kResident3 * n_cu stream-channels) and planar / interleaved layouts, against the CPU statement (orc at 1024 unlocked without a lifter,
tests/pv_ref/ref_pv.c otherwise).  A formant dimension from its own generator (the draws above stay the seed's): half the cases take a lifter
in 1 ... N/4, and every case an input level 2^-36 ... 2^20.  Returns the worst relative RMS error.
    python tests/tools/fuzz_stretch_any.py [cases=40] [seed=1]"""
import ctypes as C
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import naeload
import orc
import pv_ref

RESIDENT3 = {512: 16, 1024: 8, 2048: 6, 4096: 3}     # PvAny<N>::kResident3 (kernels_pv_any.hip)


def rel_rms(a, b):
    d = np.sqrt(np.mean((a.astype(np.float64) - b) ** 2))
    return d / max(np.sqrt(np.mean(b.astype(np.float64) ** 2)), 1e-30)


def cu_count():
    hip = C.CDLL("libamdhip64.so.7")                    # already loaded by libnae_gpu.so
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0       # hipDeviceAttributeMultiprocessorCount
    return v.value


def main(cases=40, seed=1, ctx=None, nae=None, max_samples=4_000_000):
    """max_samples bounds n_streams * L * ch and n_streams * out_len * ch of a case (a draw above it is shrunk to fewer streams)"""
    rng = np.random.default_rng(seed)
    if nae is None:
        nae = naeload.load()
    if ctx is None:
        ctx = nae.Context(0)
    tmp = tempfile.mkdtemp(prefix="fuzz_any_")
    ref = pv_ref.build(tmp)
    frng = np.random.default_rng([seed, 7])
    n_cu = cu_count()
    worst = 0.0
    for k in range(cases):
        n_fft = int(rng.choice([512, 1024, 2048, 4096]))
        lock = n_fft == 1024 and bool(rng.integers(2))
        tempo = float(np.exp(rng.uniform(np.log(1 / 64), np.log(16))))
        rho = float(np.exp(rng.uniform(np.log(1 / 16), np.log(16))))
        pitch, rate = 1 / tempo, rho * tempo
        ch = int(rng.choice([1, 2]))
        N, H = n_fft, n_fft // 4
        L = int(rng.choice([1, H - 1, H, N // 2 - 1, N // 2, N - 1, N, N + 1, N + H + 1, int(rng.integers(2, 40000))]))
        thr = RESIDENT3[n_fft] * n_cu // ch
        n_streams = int(rng.choice([1, 2, 3, 5, thr - 1, thr, thr + 1]))
        pl = ctx.stretch_plan(rate, pitch, L, n_fft)
        while L > 1 and max(L, pl.out_len) * ch > max_samples // 4:     # tempo * rho down to 1/1024: keep one stream's output short
            L //= 2
            pl = ctx.stretch_plan(rate, pitch, L, n_fft)
        while n_streams > 1 and n_streams * max(L, pl.out_len) * ch > max_samples:
            n_streams = max(1, n_streams // 4)
        planar_in, planar_out = bool(rng.integers(2)), bool(rng.integers(2))
        x = (0.5 * rng.uniform(-1, 1, (n_streams, L, ch))).astype(np.float32)
        lifter = int(frng.integers(1, N // 4 + 1)) if frng.integers(2) else 0
        level = 2.0 ** int(frng.integers(-36, 21))
        x *= np.float32(level)
        flat = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1) if planar_in else x.reshape(-1)
        d_x, d_o = ctx.array(flat), ctx.empty(max(1, n_streams * pl.out_len * ch))
        src = nae.Sig.planar(d_x.ptr, L, ch) if planar_in else nae.Sig.interleaved(d_x.ptr, L, ch)
        dst = nae.Sig.planar(d_o.ptr, pl.out_len, ch) if planar_out else nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)
        ctx.stretch_block(rate, pitch, src, L, ch, n_streams, dst, phase_lock=lock, n_fft=n_fft, formant=lifter)
        out = d_o.download()[: n_streams * pl.out_len * ch]
        out = out.reshape(n_streams, ch, pl.out_len).transpose(0, 2, 1) if planar_out else out.reshape(n_streams, pl.out_len, ch)
        d_x.free(); d_o.free()
        assert np.isfinite(out).all(), f"case {k}: non-finite output"
        errs = []
        for s in sorted({0, n_streams // 2, n_streams - 1}):
            xs = x[s].reshape(-1)
            if n_fft == 1024 and not lock and not lifter:
                want = orc.stretch(xs, ch, rate, pitch)
            else:
                want = pv_ref.stretch(ref, xs, ch, rate, pitch, n_fft, lock, lifter)
            want = want.reshape(-1, ch)
            assert want.shape == out[s].shape, (want.shape, out[s].shape)
            if want.size and np.sqrt(np.mean(want.astype(np.float64) ** 2)) >= 1e-6 * level:    # near-silent references: the edge-length rule
                errs.append(rel_rms(out[s], want))
        e = max(errs) if errs else 0.0
        worst = max(worst, e)
        flag = "" if e <= 1e-4 else "   <-- ABOVE TOLERANCE"
        print(f"case {k:3d}: N {n_fft:4d}{' lock' if lock else '     '} streams {n_streams:5d} ch {ch} L {L:6d} tempo {tempo:8.5f} rho {rho:8.5f} "
              f"{'P' if planar_in else 'I'}->{'P' if planar_out else 'I'} q {lifter:4d} level 2^{int(np.log2(level)):+d} out {pl.out_len:7d}  rel-RMS {e:.2e}{flag}", flush=True)
    print(f"worst rel-RMS {worst:.2e} over {cases} cases (tolerance 1e-4)")
    return worst


if __name__ == "__main__":
    w = main(*(int(a) for a in sys.argv[1:3]))
    sys.exit(0 if w <= 1e-4 else 1)
