#!/usr/bin/env python3
"""Times nae_fir_block_f32 (K9, the FIR filter) with nae_event_elapsed_ms: warm, the median of several runs, next to two yardsticks at the
same shape on the same device — the byte floor (8 bytes per sample per channel at the streaming rate profiles/ records) and
nae_spectrum_block_f32, which does one 512-point complex FFT per 256 samples as this filter does at n_fft = 1024.

    python tools/fir_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Shapes: 1024 stereo streams x 10 s and 16 stereo streams x 10 min at 48 kHz (--quick: 10 streams x 10 s and 16 streams x 6 s).  Every shape
is a step of nodetime.drive under --limit (default 60 s).  Prints one line per (shape, n_fft / taps) and one JSON line per shape
(profiles/r15_fir.md is written from them).
Steps: large, long (--quick: quick-large, quick-long)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000), "long": ("16 streams x 10 min", 16, 28800000),
          "quick-large": ("1024 streams x 10 s / 100", 10, 480000), "quick-long": ("16 streams x 10 min / 100", 16, 288000)}
STREAM_GBPS = 4730.0   # a 1 read : 1 write copy on this device (profiles/r04_rw_mix.md), GB/s


def steps(quick):
    return nodetime.shape_steps(quick, ("large", "long"))


def run_shape(key, runs, warmup):
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[key]
    rows, ch = [], 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        floor_ms = n_streams * T * ch * 8 / (STREAM_GBPS * 1e9) * 1e3
        F = ctx.spectrum_frames(T)
        d_spec = ctx.empty(n_streams * F * ch * 513)
        spec = nodetime.timed(ctx, lambda: ctx.spectrum_block(src, T, ch, n_streams, d_spec.ptr, F * ch * 513), runs, warmup)
        d_spec.free()
        for n_fft, L in ((1024, 513), (4096, 2049)):
            taps = nae.Context.fir_design("lowpass", 48000, 0.0, 1000.0, L)
            med, lo, hi = nodetime.timed(ctx, lambda: ctx.fir_block(taps, src, T, ch, n_streams, dst, n_fft), runs, warmup)
            rows.append({"shape": name, "n_streams": n_streams, "frames": T, "n_fft": n_fft, "taps": L, "fir_ms": med, "fir_min_ms": lo, "fir_max_ms": hi,
                         "byte_floor_ms": floor_ms, "spectrum_ms": spec[0], "gsamples_per_s": n_streams * T * ch / med / 1e6})
            print(f"{name}: n_fft {n_fft} / {L} taps: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); byte floor {floor_ms:.3f} ms "
                  f"({med / floor_ms:.1f}x); spectrum 1024 / 256 {spec[0]:.3f} ms ({med / spec[0]:.2f}x)", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    args = nodetime.parser(60.0, "a hundredth of the shapes (a smoke run of the tool)", choices=sorted(SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
