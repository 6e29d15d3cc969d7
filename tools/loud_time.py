#!/usr/bin/env python3
"""Times the loudness entries (K14): nae_loud_measure_f32 and nae_loud_normalize_f32 between two nae_event_records, warm, the median of several
runs, next to nae_eq_block_f32 with the K-weighting's two sections timed at the same shape in the same process (the cascade alone, with its
store), and the per-kernel split of one normalize from the library's own event pairs.

    python tools/loud_time.py [--runs 7] [--warmup 2] [--quick] [--shape NAME] [--only measure|normalize]

Shapes at 48 kHz stereo: 1024 streams x 10 s, 128 streams x 10 s, 1 stream x 10 min (--quick: 64 x 2 s, 8 x 2 s, 1 x 30 s).  Per case: the time
and the rate against the byte floor — 8 bytes per stereo frame read for measure, 24 for normalize (read twice, written once).  --shape and
--only cut the run down to one case (a profiler's pass).  "measure_cold" is measure with the destination buffer cleared on the stream in front of
every timed call (outside the events): what the measure kernel costs inside a normalize, whose apply has just written as many bytes as
the source has — a source of up to the 256 MiB of the chip's last-level cache stays in it from one measure call to the next, and not
across a normalize.  One JSON line at the end (profiles/r20_loud.md is written from it)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naeload  # noqa: E402
from fir_time import timed  # noqa: E402


def timed_behind(ctx, before, fn, runs, warmup):
    """as fir_time.timed, with before() queued on the stream in front of every call and outside its pair of events"""
    a, b = ctx.event(), ctx.event()
    ms = []
    for i in range(warmup + runs):
        before()
        ctx.record(a)
        fn()
        ctx.record(b)
        t = ctx.elapsed_ms(a, b)
        if i >= warmup:
            ms.append(t)
    ctx.destroy_event(a)
    ctx.destroy_event(b)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes (a smoke run of the tool)")
    ap.add_argument("--shape", default=None, help="only the shape of this name")
    ap.add_argument("--only", choices=("measure", "normalize"), default=None)
    args = ap.parse_args()
    nae = naeload.load()
    shapes = [("1024x10s", 1024, 480000), ("128x10s", 128, 480000), ("1x10min", 1, 28800000)]
    if args.quick:
        shapes = [("64x2s", 64, 96000), ("8x2s", 8, 96000), ("1x30s", 1, 1440000)]
    rows = []
    with nae.Context(0) as ctx:
        params = nae.Context.loud_design(48000)
        coef = np.array(params.coef[:]).reshape(2, 5)
        for name, n_streams, T in shapes:
            if args.shape and args.shape != name:
                continue
            ch = 2
            d_in = ctx.empty(n_streams * T * ch)
            ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
            d_out = ctx.empty(n_streams * T * ch)
            d_res = ctx.empty(n_streams * 56, np.uint8)
            src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
            frames = n_streams * T
            row = {"shape": name, "n_streams": n_streams, "frames": T}
            measure = lambda: ctx.loud_measure(params, src, T, ch, n_streams, d_res.ptr)
            cases = (("measure", 8, measure), ("measure_cold", 8, measure),
                     ("normalize", 24, lambda: ctx.loud_normalize(params, src, T, ch, n_streams, dst, d_res.ptr)),
                     ("eq2", 16, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst)))
            for what, floor_bytes, fn in cases:
                if args.only and what != args.only:
                    continue
                if what == "measure_cold":
                    med, lo, hi = timed_behind(ctx, d_out.zero, fn, args.runs, args.warmup)
                else:
                    med, lo, hi = timed(ctx, fn, args.runs, args.warmup)
                row[what + "_ms"], row[what + "_min_ms"], row[what + "_max_ms"] = med, lo, hi
                row[what + "_gbytes_per_s"] = frames * floor_bytes / med / 1e6
                print(f"{name}: {what}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {frames * floor_bytes / med / 1e6:.1f} GB/s of its "
                      f"{floor_bytes} bytes per stereo frame; {frames / med / 1e6:.2f} G frames/s", flush=True)
            if not args.only:
                ctx.prof_reset()
                ctx.prof_enable(True)
                ctx.loud_normalize(params, src, T, ch, n_streams, dst, d_res.ptr)
                ctx.sync()
                ctx.prof_enable(False)
                row["kernels_ms"] = {k: float(v[0]) for k, v in ctx.prof_report().items()}
                print(f"{name}: one normalize by kernel: {row['kernels_ms']}", flush=True)
                r = ctx.loud_results(d_res.ptr, 1)[0]
                row["stream0"] = {"lufs": r.lufs, "gain": r.gain, "true_peak": r.true_peak[0], "blocks": r.blocks_total}
            rows.append(row)
            for d in (d_in, d_out, d_res):
                d.free()
        print(json.dumps({"device": ctx.name(), "runs": args.runs, "rows": rows}))


if __name__ == "__main__":
    main()
