#!/usr/bin/env python3
"""Times nae_eq_block_f32 (K11, the biquad cascade) between two nae_event_records: warm, the median of several runs, at S = 1, 4, 8 and 16
sections, next to nae_fir_block_f32 with 513 taps (n_fft 1024) timed at the same shape in the same process.

    python tools/eq_time.py [--runs 7] [--warmup 2] [--quick]

Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Per case: the time,
the traffic rate at 8 bytes per sample and channel, the f64 operation rate at 13 operations per sample and section (zero-state pass 8,
correction 4, the scan's share 1), and the time per section, (t(S) - t(1)) / (S - 1).  One JSON line at the end (profiles/r17_eq.md is written
from it)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import naeload  # noqa: E402
from fir_time import timed  # noqa: E402

BANDS = (("peak", 1000.0, 6.0, 1.0), ("lowshelf", 120.0, -4.0, 0.707), ("highshelf", 9000.0, 3.0, 0.9), ("peak", 20.0, 12.0, 10.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the large shape's streams, and a fifth of the length")
    args = ap.parse_args()
    nae = naeload.load()
    shapes = [("1024 streams x 10 s", 1024, 480000), ("8 streams x 10 s", 8, 480000)]
    if args.quick:
        shapes = [("64 streams x 2 s", 64, 96000), ("8 streams x 2 s", 8, 96000)]
    rows = []
    with nae.Context(0) as ctx:
        for name, n_streams, T in shapes:
            ch = 2
            d_in = ctx.empty(n_streams * T * ch)
            ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
            d_out = ctx.empty(n_streams * T * ch)
            src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
            taps = nae.Context.fir_design("lowpass", 48000, 0.0, 1000.0, 513)
            fir = timed(ctx, lambda: ctx.fir_block(taps, src, T, ch, n_streams, dst, 1024), args.runs, args.warmup)[0]
            samples = n_streams * ch * T
            print(f"{name}: fir 513 taps / 1024: {fir:.3f} ms ({samples * 8 / fir / 1e6:.1f} GB/s)", flush=True)
            first = None
            for S in (1, 4, 8, 16):
                coef = np.stack([nae.Context.eq_design(BANDS[i % len(BANDS)][0], 48000, *BANDS[i % len(BANDS)][1:]) for i in range(S)])
                med, lo, hi = timed(ctx, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), args.runs, args.warmup)
                first = med if first is None else first
                per = (med - first) / (S - 1) if S > 1 else 0.0
                rows.append({"shape": name, "n_streams": n_streams, "frames": T, "sections": S, "eq_ms": med, "eq_min_ms": lo, "eq_max_ms": hi,
                             "fir_ms": fir, "ratio_to_fir": med / fir, "gbytes_per_s": samples * 8 / med / 1e6,
                             "f64_gops": samples * S * 13 / med / 1e6, "ms_per_section": per})
                print(f"{name}: S = {S}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {samples * 8 / med / 1e6:.1f} GB/s; "
                      f"{samples * S * 13 / med / 1e6:.1f} f64 Gop/s; {med / fir:.2f}x the FIR filter; {per:.3f} ms per section", flush=True)
            d_in.free()
            d_out.free()
        print(json.dumps({"device": ctx.name(), "runs": args.runs, "rows": rows}))


if __name__ == "__main__":
    main()
