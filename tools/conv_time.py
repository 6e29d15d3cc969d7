#!/usr/bin/env python3
"""Times nae_conv_block_f32 (K10, the long convolution) between two nae_event_records: warm, the median of several runs, next to
nae_fir_block_f32 at the same shape and n_fft in the same process — the same two FFTs per block with one product per bin, so the ratio is what
the ring of spectra and the sums over P partitions cost.

    python tools/conv_time.py [--runs 7] [--warmup 2] [--quick]

Shapes: 16 streams x 6 s and 1024 streams x 10 s, stereo at 48 kHz (--quick: 16 streams x 6 s and 64 streams x 2 s).  Cases: L = 2048, 24 000,
72 000 and 240 000 taps at the picked n_fft and at 4096 (one set of taps for both channels).  Prints one line per case with the ratio to the FIR
filter and the slope per partition, (conv - fir) / (P - 1), and one JSON line at the end (profiles/r16_conv.md is written from it)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naeload  # noqa: E402
from fir_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="the small shape, and a sixteenth of the large one's streams at a fifth of its length")
    args = ap.parse_args()
    nae = naeload.load()
    shapes = [("16 streams x 6 s", 16, 288000), ("1024 streams x 10 s", 1024, 480000)]
    if args.quick:
        shapes[1] = ("64 streams x 2 s", 64, 96000)
    rows = []
    rng = np.random.default_rng(1)
    with nae.Context(0) as ctx:
        for name, n_streams, T in shapes:
            ch = 2
            d_in = ctx.empty(n_streams * T * ch)
            ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
            d_out = ctx.empty(n_streams * T * ch)
            src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
            fir_ms = {}
            for L in (2048, 24000, 72000, 240000):
                taps = (rng.uniform(-1, 1, L) * np.exp(-6.9 * np.arange(L) / L)).astype(np.float32)
                for n_fft in sorted({nae.Context.conv_pick_n_fft(L), 4096}):
                    if n_fft not in fir_ms:
                        short = taps[:n_fft // 2]
                        fir_ms[n_fft] = timed(ctx, lambda: ctx.fir_block(short, src, T, ch, n_streams, dst, n_fft), args.runs, args.warmup)[0]
                    P = -(-L // (n_fft // 2))
                    med, lo, hi = timed(ctx, lambda: ctx.conv_block(taps, src, T, ch, n_streams, dst, n_fft), args.runs, args.warmup)
                    fir = fir_ms[n_fft]
                    slope = (med - fir) / (P - 1) if P > 1 else 0.0
                    rows.append({"shape": name, "n_streams": n_streams, "frames": T, "taps": L, "n_fft": n_fft, "parts": P,
                                 "picked": n_fft == nae.Context.conv_pick_n_fft(L), "conv_ms": med, "conv_min_ms": lo, "conv_max_ms": hi,
                                 "fir_ms": fir, "ratio": med / fir, "ms_per_partition": slope,
                                 "gcmac_per_s": n_streams * ch * (T / (n_fft // 2)) * (n_fft // 2 + 1) * P / med / 1e6})
                    print(f"{name}: {L} taps, n_fft {n_fft} (P = {P}): {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); fir {fir:.3f} ms "
                          f"({med / fir:.2f}x); {slope:.4f} ms per partition", flush=True)
            d_in.free()
            d_out.free()
        print(json.dumps({"device": ctx.name(), "runs": args.runs, "rows": rows}))


if __name__ == "__main__":
    main()
