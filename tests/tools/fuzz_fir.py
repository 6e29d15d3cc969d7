#!/usr/bin/env python3
"""Randomised differential run (GPU box): the FIR filter (nae_fir_block_f32 and the nae_fir handle) against the CPU statement
tests/fir_ref/ref_fir.c, bit for bit, over random frame sizes, tap counts (uniform taps or nae_fir_design's), lengths around the block
edges, channel and stream counts, views with gaps, a shared source, forced and automatic tilings and, for one case in three, the handle
with random put sizes.
    python tests/tools/fuzz_fir.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import naeload
import fir_ref
from block_gpu import bits, noise, statement
from fir_gpu import fir_stream, gpu_fir, ref_fir, ref_fir_flushed


def draw_taps(rng, nae, L):
    """uniform taps, or for an odd L of at least 3 (one time in two) a Kaiser design of random kind and corners"""
    if L >= 3 and L % 2 == 1 and rng.integers(2):
        kind = str(rng.choice(fir_ref.KINDS))
        rate = int(rng.choice([44100, 48000, 96000]))
        f_lo, f_hi = sorted(float(f) for f in rng.uniform(0.01, 0.49, 2) * rate)
        return nae.Context.fir_design(kind, rate, f_lo, f_hi + 1.0, L), kind
    return rng.uniform(-1, 1, L).astype(np.float32), "uniform"


def main(cases=60, seed=1, ctx=None, nae=None):
    rng = np.random.default_rng(seed)
    if nae is None:
        nae = naeload.load()
    if ctx is None:
        ctx = nae.Context(0)
    ref = statement(fir_ref)
    done = 0
    try:
        for k in range(cases):
            n_fft = int(rng.choice(fir_ref.SIZES))
            B = n_fft // 2
            L = int(rng.choice([1, 2, 3, B - 1, B, B + 1, int(rng.integers(1, B + 2)), int(rng.integers(1, B + 2))]))
            taps, kind = draw_taps(rng, nae, L)
            kb = int(rng.integers(1, 12))
            in_len = max(1, int(rng.choice([1, B - 1, B + 1, kb * B, kb * B - 1, kb * B + 1, int(rng.integers(1, 70 * B + 1))])))
            ch = int(rng.integers(1, 3))
            blocks = -(-in_len // B)
            tile = int(rng.choice([0, 1, int(rng.integers(1, blocks + 3))]))
            ctx.debug_set("fir_tile", tile)
            if k % 3 == 2:
                x = noise(rng, 1, in_len, ch)[0]
                puts = [int(p) for p in rng.integers(1, 6 * B, int(rng.integers(1, 6)))]
                device = bool(rng.integers(2))
                got = fir_stream(nae, ctx, taps, n_fft, x, puts, device=device)
                want = ref_fir_flushed(ref, taps, n_fft, x)
                what = f"handle puts {puts[:3]} {'device' if device else 'host'}"
            else:
                n_streams = int(rng.integers(1, 13))
                while n_streams > 1 and n_streams * in_len * ch > 1 << 21:     # keep a case's signal to 8 MiB
                    n_streams //= 2
                sl, dl = str(rng.choice(["i", "p"])), str(rng.choice(["i", "p"]))
                shared = bool(rng.integers(4) == 0)
                gap, chan_pad, offset = (int(rng.choice([0, 1, 37])) for _ in range(3))
                x = noise(rng, n_streams, in_len, ch, shared)
                got = gpu_fir(nae, ctx, taps, n_fft, x, sl, dl, shared, gap=gap, offset=offset, chan_pad=chan_pad)
                want = ref_fir(ref, taps, n_fft, x)
                what = f"block {n_streams} streams {sl}{dl}{' shared' if shared else ''} gap {gap} pad {chan_pad} offset {offset}"
            assert got.shape == want.shape, (k, got.shape, want.shape)
            assert np.array_equal(bits(got), bits(want)), f"case {k}: n_fft {n_fft} L {L} {kind} in_len {in_len} ch {ch} tile {tile} {what}: differs"
            done += 1
            print(f"case {k:3d}: n_fft {n_fft:4d} L {L:4d} {kind:8s} in_len {in_len:6d} ch {ch} tile {tile:2d} {what}  bit-exact", flush=True)
    finally:
        ctx.debug_set("fir_tile", 0)
    print(f"{done} cases bit-exact")
    return done


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
