#!/usr/bin/env python3
"""Times nae_eq_block_f32 (K11, the biquad cascade) between two nae_event_records: warm, the median of several runs, at S = 1, 4, 8 and 16
sections, next to nae_fir_block_f32 with 513 taps (n_fft 1024) timed at the same shape in the same process.

    python tools/eq_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a
step of nodetime.drive under --limit (default 60 s).  Per case: the time, the traffic rate at 8 bytes per sample and channel, the f64
operation rate at 13 operations per sample and section (zero-state pass 8, correction 4, the scan's share 1), and the time per section,
(t(S) - t(1)) / (S - 1).  One JSON line per shape (profiles/r17_eq.md is written from them).
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps
BANDS = (("peak", 1000.0, 6.0, 1.0), ("lowshelf", 120.0, -4.0, 0.707), ("highshelf", 9000.0, 3.0, 0.9), ("peak", 20.0, 12.0, 10.0))


def run_shape(key, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[key]
    rows, ch = [], 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        taps = nae.Context.fir_design("lowpass", 48000, 0.0, 1000.0, 513)
        fir = nodetime.timed(ctx, lambda: ctx.fir_block(taps, src, T, ch, n_streams, dst, 1024), runs, warmup)[0]
        samples = n_streams * ch * T
        print(f"{name}: fir 513 taps / 1024: {fir:.3f} ms ({samples * 8 / fir / 1e6:.1f} GB/s)", flush=True)
        first = None
        for S in (1, 4, 8, 16):
            coef = np.stack([nae.Context.eq_design(BANDS[i % len(BANDS)][0], 48000, *BANDS[i % len(BANDS)][1:]) for i in range(S)])
            med, lo, hi = nodetime.timed(ctx, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), runs, warmup)
            first = med if first is None else first
            per = (med - first) / (S - 1) if S > 1 else 0.0
            rows.append({"shape": name, "n_streams": n_streams, "frames": T, "sections": S, "eq_ms": med, "eq_min_ms": lo, "eq_max_ms": hi,
                         "fir_ms": fir, "ratio_to_fir": med / fir, "gbytes_per_s": samples * 8 / med / 1e6,
                         "f64_gops": samples * S * 13 / med / 1e6, "ms_per_section": per})
            print(f"{name}: S = {S}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {samples * 8 / med / 1e6:.1f} GB/s; "
                  f"{samples * S * 13 / med / 1e6:.1f} f64 Gop/s; {med / fir:.2f}x the FIR filter; {per:.3f} ms per section", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    args = nodetime.parser(60.0, choices=sorted(nodetime.SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
