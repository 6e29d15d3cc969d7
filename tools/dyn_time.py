#!/usr/bin/env python3
"""Times nae_dyn_block_f32 (K12, the dynamics processor) between two nae_event_records: warm, the median of several runs, at look-aheads of
0, 15, 64 and 1024 samples, linked and unlinked, next to nae_eq_block_f32 with four sections timed at the same shape in the same process.

    python tools/dyn_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a
step of its own: a fresh child process (this file with --shape) under a time limit of --limit seconds (default 120), and the first step that
fails or runs out of time ends the run with its exit status; nothing more is started on the device after it.  Per case: the time, the traffic
rate at 8 bytes per sample and channel (12 with the second read of the samples at the gain stage, which the caches are expected to serve),
and the f64 operation rate at 90 operations per detector sample (level 40 with the division's 12, curve 6, look-ahead 3, release 10, attack 7,
gain 27; counted from the source).  One JSON line per shape (profiles/r18_dyn.md is written from them)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000), "small": ("8 streams x 10 s", 8, 480000),
          "quick-large": ("64 streams x 2 s", 64, 96000), "quick-small": ("8 streams x 2 s", 8, 96000)}
OPS_PER_SAMPLE = 90


def run_shape(key, runs, warmup):
    import numpy as np
    import naeload
    from fir_time import timed
    nae = naeload.load()
    name, n_streams, T = SHAPES[key]
    rows, ch = [], 2
    with nae.Context(0) as ctx:
        d_in = ctx.empty(n_streams * T * ch)
        ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
        d_out = ctx.empty(n_streams * T * ch)
        src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
        coef = np.stack([nae.Context.eq_design("peak", 48000, f, 3.0, 1.0) for f in (100.0, 1000.0, 4000.0, 9000.0)])
        eq = timed(ctx, lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst), runs, warmup)[0]
        samples = n_streams * ch * T
        print(f"{name}: eq, 4 sections: {eq:.3f} ms ({samples * 8 / eq / 1e6:.1f} GB/s)", flush=True)
        for link in (1, 0):
            for la in (0, 15, 64, 1024):
                p = nae.Context.dyn_design(48000, -18.0, 4.0, 6.0, 0.005, 0.1, la / 48000.0, 0.0, link)
                assert p.lookahead == la
                med, lo, hi = timed(ctx, lambda: ctx.dyn_block(p, src, T, ch, n_streams, dst), runs, warmup)
                det = samples // 2 if link else samples
                rows.append({"shape": name, "n_streams": n_streams, "frames": T, "link": link, "lookahead": la, "dyn_ms": med, "dyn_min_ms": lo,
                             "dyn_max_ms": hi, "eq4_ms": eq, "ratio_to_eq4": med / eq, "gbytes_per_s": samples * 8 / med / 1e6,
                             "f64_gops": det * OPS_PER_SAMPLE / med / 1e6})
                print(f"{name}: link {link}, look-ahead {la}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {samples * 8 / med / 1e6:.1f} GB/s; "
                      f"{det * OPS_PER_SAMPLE / med / 1e6:.1f} f64 Gop/s; {med / eq:.2f}x the 4-section equalizer", flush=True)
        d_in.free()
        d_out.free()
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the large shape's streams, and a fifth of the length")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each shape's process may take")
    ap.add_argument("--shape", choices=sorted(SHAPES), help="run this one shape in this process (what the driver starts)")
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    for key in (("quick-large", "quick-small") if args.quick else ("large", "small")):
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", key, "--runs", str(args.runs), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{key}: no result within {args.limit:g} s; stopping", flush=True)
            return 124
        if rc:
            print(f"{key}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
