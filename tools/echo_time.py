#!/usr/bin/env python3
"""Times nae_echo_block_f32 (K16, the echo) next to nae_eq_block_f32, between two nae_event_records: warm, interleaved (every round times
every case once, in turn), the median over the rounds, with the shader clock read before and after.

    python tools/echo_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz:
  a  nae_eq_block_f32, two sections (a low-pass and a high-pass): the same arithmetic at 8 bytes per sample
  b  the echo at D = 350 ms, the same two sections in the loop: 16 bytes per sample (the signal in and out, the line out and in)
  c  b with ping-pong and delays of 350 and 250 ms
  d  the echo with no section
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a step of
nodetime.drive under --limit (default 180 s).  One JSON line per shape
(profiles/r22_echo.md is written from them).
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
        plain = nae.Context.echo_design(48000, 0.35, None, 0.4, 4000.0, 100.0, 0.35, 1.0, False)
        pong = nae.Context.echo_design(48000, 0.35, 0.25, 0.4, 4000.0, 100.0, 0.35, 1.0, True)
        bare = nae.Context.echo_design(48000, 0.35, None, 0.4, 0.0, 0.0, 0.35, 1.0, False)
        coef = np.array([[plain.coef[s][i] for i in range(5)] for s in range(2)])
        signal = n_streams * ch * T * 4
        cases = (("a", "nae_eq_block_f32, 2 sections", lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), 2 * signal),
                 ("b", "echo, 350 ms, 2 sections", lambda: ctx.echo_block(plain, src, T, ch, n_streams, dst), 4 * signal),
                 ("c", "echo, ping-pong 350 / 250 ms, 2 sections", lambda: ctx.echo_block(pong, src, T, ch, n_streams, dst), 4 * signal),
                 ("d", "echo, 350 ms, no section", lambda: ctx.echo_block(bare, src, T, ch, n_streams, dst), 4 * signal))
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        rows = []
        for tag, what, _, traffic in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "bytes": traffic, "gbytes_per_s": traffic / med / 1e6})
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: b/a {t['b'] / t['a']:.3f} (traffic 2), c/a {t['c'] / t['a']:.3f}, d/a {t['d'] / t['a']:.3f}; "
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
