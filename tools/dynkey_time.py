#!/usr/bin/env python3
"""Times nae_dynkey_block_f32 (K15, the keyed dynamics) against what it stands beside and what it replaces, between two nae_event_records:
warm, interleaved (every round times every case once, in turn), the median over the rounds.

    python tools/dynkey_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, linked stereo at a look-ahead of 64 samples:
  a  nae_dyn_block_f32
  b  keyed, no section, an external stereo key
  c  keyed, no section, one mono key shared by every stream (stream_stride = 0)
  d  keyed, the signal its own key, two sections (a high-pass and a bell)
  e  nae_eq_block_f32 of the signal into a scratch key, then b on it: the composition d replaces
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a
step of its own: a fresh child process (this file with --shape) under a time limit of --limit seconds (default 180), and the first step that
fails or runs out of time ends the run with its exit status; nothing more is started on the device after it.  Traffic is counted at 4 bytes
per sample read or written once: the signal in and out, and the key where it is another signal.  One JSON line per shape
(profiles/r21_dynkey.md is written from them)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000), "small": ("8 streams x 10 s", 8, 480000),
          "quick-large": ("64 streams x 2 s", 64, 96000), "quick-small": ("8 streams x 2 s", 8, 96000)}


def run_shape(shape, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_key, d_scratch, d_out = (ctx.empty(n_streams * T * ch) for _ in range(4))
        ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
        ctx.fill_uniform(d_key.ptr, T * ch, T * ch, n_streams, 0, 1)
        src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
        key2, scratch = nae.Sig.interleaved(d_key.ptr, T, ch), nae.Sig.interleaved(d_scratch.ptr, T, ch)
        key1 = nae.Sig(d_key.ptr, 0, 1, 1)
        dyn = nae.Context.dyn_design(48000, -18.0, 4.0, 6.0, 0.005, 0.1, 64 / 48000.0, 0.0, 1)
        coef = np.stack([nae.Context.eq_design("highpass", 48000, 150.0, 0.0, 0.7071), nae.Context.eq_design("peak", 48000, 3000.0, 6.0, 1.0)])
        ext2, ext1 = nae.DynKeyParams.make(dyn, 2), nae.DynKeyParams.make(dyn, 1)
        own2 = nae.DynKeyParams.make(dyn, 0, coef)

        def composed():
            ctx.eq_block(coef, src, T, ch, n_streams, scratch)
            ctx.dynkey_block(ext2, src, scratch, T, ch, n_streams, dst)

        signal = n_streams * ch * T * 4
        cases = (("a", "nae_dyn_block_f32", lambda: ctx.dyn_block(dyn, src, T, ch, n_streams, dst), 2 * signal),
                 ("b", "keyed, 0 sections, stereo key", lambda: ctx.dynkey_block(ext2, src, key2, T, ch, n_streams, dst), 3 * signal),
                 ("c", "keyed, 0 sections, one shared mono key", lambda: ctx.dynkey_block(ext1, src, key1, T, ch, n_streams, dst), 2 * signal + T * 4),
                 ("d", "keyed, own key, 2 sections", lambda: ctx.dynkey_block(own2, src, None, T, ch, n_streams, dst), 2 * signal),
                 ("e", "nae_eq_block_f32 into a key, then b", composed, 5 * signal))
        a, b = ctx.event(), ctx.event()
        for _ in range(warmup):
            for _, _, fn, _ in cases:
                fn()
        ctx.sync()
        ms = {c[0]: [] for c in cases}
        for _ in range(runs):
            for tag, _, fn, _ in cases:
                ctx.record(a)
                fn()
                ctx.record(b)
                ms[tag].append(ctx.elapsed_ms(a, b))
        ctx.destroy_event(a)
        ctx.destroy_event(b)
        rows = []
        for tag, what, _, traffic in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "bytes": traffic, "gbytes_per_s": traffic / med / 1e6})
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: b/a {t['b'] / t['a']:.3f} (traffic 3/2), c/a {t['c'] / t['a']:.3f}, d/a {t['d'] / t['a']:.3f}, d/e {t['d'] / t['e']:.3f}", flush=True)
        for d in (d_in, d_key, d_scratch, d_out):
            d.free()
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the large shape's streams, and a fifth of the length")
    ap.add_argument("--limit", type=float, default=180.0, help="seconds each shape's process may take")
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
