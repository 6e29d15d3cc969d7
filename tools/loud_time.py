#!/usr/bin/env python3
"""Times the loudness entries (K14): nae_loud_measure_f32 and nae_loud_normalize_f32 between two nae_event_records, warm, the median of several
runs, next to nae_eq_block_f32 with the K-weighting's two sections timed at the same shape in the same process (the cascade alone, with its
store), and the per-kernel split of one normalize from the library's own event pairs.

    python tools/loud_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS] [--shape NAME] [--only measure|normalize]

Shapes at 48 kHz stereo: 1024 streams x 10 s, 128 streams x 10 s, 1 stream x 10 min (--quick: 64 x 2 s, 8 x 2 s, 1 x 30 s).  Per case: the time
and the rate against the byte floor — 8 bytes per stereo frame read for measure, 24 for normalize (read twice, written once).  --shape and
--only cut the run down to one case in this process (a profiler's pass); without --shape every shape is a step of nodetime.drive under
--limit (default 60 s).  "measure_cold" is measure with the destination buffer cleared on the stream in front of
every timed call (outside the events): what the measure kernel costs inside a normalize, whose apply has just written as many bytes as
the source has — a source of up to the 256 MiB of the chip's last-level cache stays in it from one measure call to the next, and not
across a normalize.  One JSON line per shape (profiles/r20_loud.md is written from them).
Steps: 1024x10s, 128x10s, 1x10min (--quick: 64x2s, 8x2s, 1x30s)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

SHAPES = {"1024x10s": (1024, 480000), "128x10s": (128, 480000), "1x10min": (1, 28800000),
          "64x2s": (64, 96000), "8x2s": (8, 96000), "1x30s": (1, 1440000)}


def steps(quick):
    return [(name, ["--shape", name]) for name in (("64x2s", "8x2s", "1x30s") if quick else ("1024x10s", "128x10s", "1x10min"))]


def run_shape(name, runs, warmup, only):
    import numpy as np
    import naeload
    nae = naeload.load()
    n_streams, T = SHAPES[name]
    ch = 2
    with nae.Context(0) as ctx:
        params = nae.Context.loud_design(48000)
        coef = np.array(params.coef[:]).reshape(2, 5)
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        d_res = ctx.empty(n_streams * 56, np.uint8)
        frames = n_streams * T
        row = {"shape": name, "n_streams": n_streams, "frames": T}
        measure = lambda: ctx.loud_measure(params, src, T, ch, n_streams, d_res.ptr)
        cases = (("measure", 8, measure), ("measure_cold", 8, measure),
                 ("normalize", 24, lambda: ctx.loud_normalize(params, src, T, ch, n_streams, dst, d_res.ptr)),
                 ("eq2", 16, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst)))
        for what, floor_bytes, fn in cases:
            if only and what != only:
                continue
            if what == "measure_cold":
                med, lo, hi = nodetime.timed_behind(ctx, d_out.zero, fn, runs, warmup)
            else:
                med, lo, hi = nodetime.timed(ctx, fn, runs, warmup)
            row[what + "_ms"], row[what + "_min_ms"], row[what + "_max_ms"] = med, lo, hi
            row[what + "_gbytes_per_s"] = frames * floor_bytes / med / 1e6
            print(f"{name}: {what}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {frames * floor_bytes / med / 1e6:.1f} GB/s of its "
                  f"{floor_bytes} bytes per stereo frame; {frames / med / 1e6:.2f} G frames/s", flush=True)
        if not only:
            ctx.prof_reset()
            ctx.prof_enable(True)
            ctx.loud_normalize(params, src, T, ch, n_streams, dst, d_res.ptr)
            ctx.sync()
            ctx.prof_enable(False)
            row["kernels_ms"] = {k: float(v[0]) for k, v in ctx.prof_report().items()}
            print(f"{name}: one normalize by kernel: {row['kernels_ms']}", flush=True)
            r = ctx.loud_results(d_res.ptr, 1)[0]
            row["stream0"] = {"lufs": r.lufs, "gain": r.gain, "true_peak": r.true_peak[0], "blocks": r.blocks_total}
        nodetime.release(d_in, d_out, d_res)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": [row]}), flush=True)


def main():
    ap = nodetime.parser(60.0, "small shapes (a smoke run of the tool)", choices=sorted(SHAPES))
    ap.add_argument("--only", choices=("measure", "normalize"), default=None)
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup, args.only)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args) + (["--only", args.only] if args.only else []))


if __name__ == "__main__":
    sys.exit(main())
