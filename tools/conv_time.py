#!/usr/bin/env python3
"""Times nae_conv_block_f32 (K10, the long convolution) between two nae_event_records: warm, the median of several runs, next to
nae_fir_block_f32 at the same shape and n_fft in the same process — the same two FFTs per block with one product per bin, so the ratio is what
the ring of spectra and the sums over P partitions cost.

    python tools/conv_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Shapes: 16 streams x 6 s and 1024 streams x 10 s, stereo at 48 kHz (--quick: 16 streams x 6 s and 64 streams x 2 s).  Every shape is a step of
nodetime.drive under --limit (default 60 s).  Cases: L = 2048, 24 000, 72 000 and 240 000 taps at the picked n_fft and at 4096 (one set
of taps for both channels).  Prints one line per case with the ratio to the FIR filter and the slope per partition, (conv - fir) / (P - 1),
and one JSON line per shape (profiles/r16_conv.md is written from them).
Steps: small, large (--quick: small, quick-large)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

SHAPES = {"small": ("16 streams x 6 s", 16, 288000), "large": ("1024 streams x 10 s", 1024, 480000), "quick-large": ("64 streams x 2 s", 64, 96000)}


def steps(quick):
    return [(k, ["--shape", k]) for k in ("small", "quick-large" if quick else "large")]


def run_shape(key, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[key]
    rows, ch = [], 2
    rng = np.random.default_rng(1)
    for _ in range(1 if key == "small" else 2):    # a run's second shape has the generator's second set of taps
        all_taps = {L: (rng.uniform(-1, 1, L) * np.exp(-6.9 * np.arange(L) / L)).astype(np.float32) for L in (2048, 24000, 72000, 240000)}
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        fir_ms = {}
        for L, taps in all_taps.items():
            for n_fft in sorted({nae.Context.conv_pick_n_fft(L), 4096}):
                if n_fft not in fir_ms:
                    short = taps[:n_fft // 2]
                    fir_ms[n_fft] = nodetime.timed(ctx, lambda: ctx.fir_block(short, src, T, ch, n_streams, dst, n_fft), runs, warmup)[0]
                P = -(-L // (n_fft // 2))
                med, lo, hi = nodetime.timed(ctx, lambda: ctx.conv_block(taps, src, T, ch, n_streams, dst, n_fft), runs, warmup)
                fir = fir_ms[n_fft]
                slope = (med - fir) / (P - 1) if P > 1 else 0.0
                rows.append({"shape": name, "n_streams": n_streams, "frames": T, "taps": L, "n_fft": n_fft, "parts": P,
                             "picked": n_fft == nae.Context.conv_pick_n_fft(L), "conv_ms": med, "conv_min_ms": lo, "conv_max_ms": hi,
                             "fir_ms": fir, "ratio": med / fir, "ms_per_partition": slope,
                             "gcmac_per_s": n_streams * ch * (T / (n_fft // 2)) * (n_fft // 2 + 1) * P / med / 1e6})
                print(f"{name}: {L} taps, n_fft {n_fft} (P = {P}): {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); fir {fir:.3f} ms "
                      f"({med / fir:.2f}x); {slope:.4f} ms per partition", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    args = nodetime.parser(60.0, "the small shape, and a sixteenth of the large one's streams at a fifth of its length", choices=sorted(SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
