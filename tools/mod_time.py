#!/usr/bin/env python3
"""Times nae_mod_block_f32 (K17, the modulated delay) next to nae_echo_block_f32 and nae_eq_block_f32, between two nae_event_records: warm,
interleaved (every round times every case once, in turn), the median over the rounds, with the shader clock read before and after.

    python tools/mod_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz:
  a  nae_eq_block_f32, two sections (a low-pass and a high-pass): 8 bytes per sample
  b  the echo at D = 350 ms with the same two sections in the loop: 16 bytes per sample
  c  the default chorus: 12 ms +- 3 ms at 0.8 Hz, three voices, no feedback (runs of 64 samples): 8 bytes per sample, 16 per stereo frame
  d  a flanger at runs of 64: delay 144, depth 48 samples, 0.25 Hz, feedback 0.7, one voice
  e  the same flanger at runs of 16: delay 24, depth 7 samples
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a step of
nodetime.drive under --limit (default 180 s).  One JSON line per shape
(profiles/r23_mod.md is written from them).
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps


def run_shape(shape, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        echo = nae.Context.echo_design(48000, 0.35, None, 0.4, 4000.0, 100.0, 0.35, 1.0, False)
        coef = np.array([[echo.coef[s][i] for i in range(5)] for s in range(2)])
        chorus = nae.Context.mod_design(48000)
        quarter_hz = nae.Context.mod_design(48000, rate_hz=0.25).rate_inc
        flanger = lambda delay, depth: nae.ModParams.make(delay, depth, 0.7, 0.7, 1.0, quarter_hz, 0, 1 << 30, (0,), 0)
        wide, narrow = flanger(144.0, 48.0), flanger(24.0, 7.0)
        signal = n_streams * ch * T * 4
        cases = (("a", "nae_eq_block_f32, 2 sections", lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), 2 * signal),
                 ("b", "echo, 350 ms, 2 sections", lambda: ctx.echo_block(echo, src, T, ch, n_streams, dst), 4 * signal),
                 ("c", "chorus, 3 voices, no feedback, runs of 64", lambda: ctx.mod_block(chorus, src, T, ch, n_streams, dst), 2 * signal),
                 ("d", "flanger (144, 48), feedback 0.7, runs of 64", lambda: ctx.mod_block(wide, src, T, ch, n_streams, dst), 2 * signal),
                 ("e", "flanger (24, 7), feedback 0.7, runs of 16", lambda: ctx.mod_block(narrow, src, T, ch, n_streams, dst), 2 * signal))
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        rows = []
        for tag, what, _, traffic in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "bytes": traffic, "gbytes_per_s": traffic / med / 1e6})
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: c/a {t['c'] / t['a']:.3f}, d/a {t['d'] / t['a']:.3f}, e/a {t['e'] / t['a']:.3f}, e/d {t['e'] / t['d']:.3f}, c/b {t['c'] / t['b']:.3f}; "
              f"clock {clock_before:.3f} GHz before, {clock_after:.3f} GHz after", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": [clock_before, clock_after], "rows": rows}), flush=True)


def main():
    args = nodetime.parser(180.0, choices=sorted(nodetime.SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
