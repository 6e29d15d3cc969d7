#!/usr/bin/env python3
"""Times nae_dyn_block_f32 (K12, the dynamics processor) between two nae_event_records: warm, the median of several runs, at look-aheads of
0, 15, 64 and 1024 samples, linked and unlinked, next to nae_eq_block_f32 with four sections timed at the same shape in the same process.

    python tools/dyn_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is
a step of nodetime.drive under --limit (default 120 s).  Per case: the time, the traffic rate at 8 bytes per sample and channel (12 with the
second read of the samples at the gain stage, which the caches are expected to serve), and the f64 operation rate at 90 operations per detector sample (level 40 with the division's 12, curve 6, look-ahead 3, release 10, attack 7,
gain 27; counted from the source).  One JSON line per shape (profiles/r18_dyn.md is written from them).
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps
OPS_PER_SAMPLE = 90


def run_shape(key, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[key]
    rows, ch = [], 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        coef = np.stack([nae.Context.eq_design("peak", 48000, f, 3.0, 1.0) for f in (100.0, 1000.0, 4000.0, 9000.0)])
        eq = nodetime.timed(ctx, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), runs, warmup)[0]
        samples = n_streams * ch * T
        print(f"{name}: eq, 4 sections: {eq:.3f} ms ({samples * 8 / eq / 1e6:.1f} GB/s)", flush=True)
        for link in (1, 0):
            for la in (0, 15, 64, 1024):
                p = nae.Context.dyn_design(48000, -18.0, 4.0, 6.0, 0.005, 0.1, la / 48000.0, 0.0, link)
                assert p.lookahead == la
                med, lo, hi = nodetime.timed(ctx, lambda: ctx.dyn_block(p, src, T, ch, n_streams, dst), runs, warmup)
                det = samples // 2 if link else samples
                rows.append({"shape": name, "n_streams": n_streams, "frames": T, "link": link, "lookahead": la, "dyn_ms": med, "dyn_min_ms": lo,
                             "dyn_max_ms": hi, "eq4_ms": eq, "ratio_to_eq4": med / eq, "gbytes_per_s": samples * 8 / med / 1e6,
                             "f64_gops": det * OPS_PER_SAMPLE / med / 1e6})
                print(f"{name}: link {link}, look-ahead {la}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {samples * 8 / med / 1e6:.1f} GB/s; "
                      f"{det * OPS_PER_SAMPLE / med / 1e6:.1f} f64 Gop/s; {med / eq:.2f}x the 4-section equalizer", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    args = nodetime.parser(120.0, choices=sorted(nodetime.SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
