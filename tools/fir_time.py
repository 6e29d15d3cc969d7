#!/usr/bin/env python3
"""Times nae_fir_block_f32 (K9, the FIR filter) with nae_event_elapsed_ms: warm, the median of several runs, next to two yardsticks at the
same shape on the same device — the byte floor (8 bytes per sample per channel at the streaming rate profiles/ records) and
nae_spectrum_block_f32, which does one 512-point complex FFT per 256 samples as this filter does at n_fft = 1024.

    python tools/fir_time.py [--runs 7] [--warmup 2] [--quick]

Prints one line per (shape, n_fft / taps) and one JSON line at the end (profiles/r15_fir.md is written from it)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naeload  # noqa: E402

STREAM_GBPS = 4730.0   # a 1 read : 1 write copy on this device (profiles/r04_rw_mix.md), GB/s


def timed(ctx, fn, runs, warmup):
    a, b = ctx.event(), ctx.event()
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(runs):
        ctx.record(a)
        fn()
        ctx.record(b)
        ms.append(ctx.elapsed_ms(a, b))
    ctx.destroy_event(a)
    ctx.destroy_event(b)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a hundredth of the shapes (a smoke run of the tool)")
    args = ap.parse_args()
    nae = naeload.load()
    shapes = [("1024 streams x 10 s", 1024, 480000), ("16 streams x 10 min", 16, 28800000)]
    if args.quick:
        shapes = [(name + " / 100", max(n // 100, 1) if n > 16 else n, T if n > 16 else T // 100) for name, n, T in shapes]
    rows = []
    with nae.Context(0) as ctx:
        for name, n_streams, T in shapes:
            ch = 2
            d_in = ctx.empty(n_streams * T * ch)
            ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
            d_out = ctx.empty(n_streams * T * ch)
            src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
            floor_ms = n_streams * T * ch * 8 / (STREAM_GBPS * 1e9) * 1e3
            F = ctx.spectrum_frames(T)
            d_spec = ctx.empty(n_streams * F * ch * 513)
            spec = timed(ctx, lambda: ctx.spectrum_block(src, T, ch, n_streams, d_spec.ptr, F * ch * 513), args.runs, args.warmup)
            d_spec.free()
            for n_fft, L in ((1024, 513), (4096, 2049)):
                taps = nae.Context.fir_design("lowpass", 48000, 0.0, 1000.0, L)
                med, lo, hi = timed(ctx, lambda: ctx.fir_block(taps, src, T, ch, n_streams, dst, n_fft), args.runs, args.warmup)
                row = {"shape": name, "n_streams": n_streams, "frames": T, "n_fft": n_fft, "taps": L, "fir_ms": med, "fir_min_ms": lo, "fir_max_ms": hi,
                       "byte_floor_ms": floor_ms, "spectrum_ms": spec[0], "gsamples_per_s": n_streams * T * ch / med / 1e6}
                rows.append(row)
                print(f"{name}: n_fft {n_fft} / {L} taps: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); byte floor {floor_ms:.3f} ms "
                      f"({med / floor_ms:.1f}x); spectrum 1024 / 256 {spec[0]:.3f} ms ({med / spec[0]:.2f}x)")
            d_in.free()
            d_out.free()
        print(json.dumps({"device": ctx.name(), "runs": args.runs, "rows": rows}))


if __name__ == "__main__":
    main()
