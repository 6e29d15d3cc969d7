#!/usr/bin/env python3
"""Times nae_hpss_block_f32 (K21, the harmonic/percussive separation) with the soft and the hard mask at spans 8 next to nae_denoise_block_f32
(K13, the spectral gate) with time_smooth 8 at the same frame size and shape, between two nae_event_records: warm, interleaved (every round
times every case once, in turn), the median over the rounds, with the shader clock read before and after.

    python tools/hpss_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS] [--sizes 512,1024,2048,4096]

Shape: 1024 stereo streams x 10 s at 48 kHz of uniform noise (--quick: 64 streams x 2 s), the library's own tile.  K13 runs against the
profile it learns from the first half second of stream 0, at the node's sensitivity.  Every frame size is a step of its own: a fresh child
process (this file with --n-fft) under a time limit of --limit seconds (default 180), and the first step that fails or runs out of time ends
the run with its exit status; nothing more is started on the device after it.  Per case: the time, the traffic rate at the 8 bytes per sample
and channel the call must move, and the ratio to K13.  One JSON line per frame size (profiles/r33_hpss.md is written from them)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {False: ("1024 streams x 10 s", 1024, 480000), True: ("64 streams x 2 s", 64, 96000)}


def run_size(n_fft, quick, runs, warmup):
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[quick]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out = ctx.empty(n_streams * T * ch), ctx.empty(n_streams * T * ch)
        ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
        d_prof = ctx.empty(ch * (n_fft // 2 + 1))
        src, dst = nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)
        ctx.denoise_profile(n_fft, src, 24000, ch, d_prof.ptr)
        gate = nae.Context.denoise_design(12.0, 6.0, n_fft, 8, 4)
        cases = [("K13", "nae_denoise_block_f32, time_smooth 8, freq_smooth 4", lambda: ctx.denoise_block(gate, d_prof.ptr, ch, src, T, ch, n_streams, dst))]
        for mask in nae.HPSS_MASKS:
            p = nae.Context.hpss_design(0.0, -120.0, n_fft, 8, 8, mask)
            cases.append((f"K21 {mask}", f"nae_hpss_block_f32, spans 8, {mask} mask", lambda p=p: ctx.hpss_block(p, src, T, ch, n_streams, dst)))
        a, b = ctx.event(), ctx.event()
        for _ in range(warmup):
            for _, _, fn in cases:
                fn()
        ctx.sync()
        clock_before = ctx.clock_ghz()
        ms = {c[0]: [] for c in cases}
        for _ in range(runs):
            for tag, _, fn in cases:
                ctx.record(a)
                fn()
                ctx.record(b)
                ms[tag].append(ctx.elapsed_ms(a, b))
        clock_after = ctx.clock_ghz()
        ctx.destroy_event(a)
        ctx.destroy_event(b)
        samples = n_streams * ch * T
        base = statistics.median(ms["K13"])
        rows = []
        for tag, what, _ in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "n_fft": n_fft, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "gbytes_per_s": samples * 8 / med / 1e6, "ratio_to_k13": med / base})
            print(f"{name}, n_fft {n_fft}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); "
                  f"{samples * 8 / med / 1e6:.1f} GB/s; {med / base:.2f} x K13", flush=True)
        d_in.free()
        d_out.free()
        d_prof.free()
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": [clock_before, clock_after], "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the streams, and a fifth of the length")
    ap.add_argument("--limit", type=float, default=180.0, help="seconds each frame size's process may take")
    ap.add_argument("--sizes", default="512,1024,2048,4096", help="the frame sizes, comma separated")
    ap.add_argument("--n-fft", type=int, help="run this one frame size in this process (what the driver starts)")
    args = ap.parse_args()
    if args.n_fft:
        run_size(args.n_fft, args.quick, args.runs, args.warmup)
        return 0
    for n_fft in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--n-fft", n_fft, "--runs", str(args.runs), "--warmup", str(args.warmup)] + (["--quick"] if args.quick else [])
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"n_fft {n_fft}: no result within {args.limit:g} s; stopping", flush=True)
            return 124
        if rc:
            print(f"n_fft {n_fft}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
