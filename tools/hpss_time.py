#!/usr/bin/env python3
"""Times nae_hpss_block_f32 (K21, the harmonic/percussive separation) with the soft and the hard mask at spans 8 next to nae_denoise_block_f32
(K13, the spectral gate) with time_smooth 8 at the same frame size and shape, between two nae_event_records: warm, interleaved (every round
times every case once, in turn), the median over the rounds, with the shader clock read before and after.

    python tools/hpss_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS] [--sizes 512,1024,2048,4096]

Shape: 1024 stereo streams x 10 s at 48 kHz of uniform noise (--quick: 64 streams x 2 s), the library's own tile.  K13 runs against the
profile it learns from the first half second of stream 0, at the node's sensitivity.  Every frame size is a step of nodetime.drive under
--limit (default 180 s).  Per case: the time, the traffic rate at the 8 bytes per sample and channel the call must move, and the ratio to
K13.  One JSON line per frame size (profiles/r33_hpss.md is written from them).
Steps: n_fft 512, n_fft 1024, n_fft 2048, n_fft 4096 (--quick: n_fft 512, n_fft 1024, n_fft 2048, n_fft 4096)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

SHAPES = {False: ("1024 streams x 10 s", 1024, 480000), True: ("64 streams x 2 s", 64, 96000)}


def steps(quick, sizes="512,1024,2048,4096"):
    return [(f"n_fft {n_fft}", ["--n-fft", n_fft] + (["--quick"] if quick else [])) for n_fft in sizes.split(",")]


def run_size(n_fft, quick, runs, warmup):
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[quick]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        d_prof = ctx.empty(ch * (n_fft // 2 + 1))
        ctx.denoise_profile(n_fft, src, 24000, ch, d_prof.ptr)
        gate = nae.Context.denoise_design(12.0, 6.0, n_fft, 8, 4)
        cases = [("K13", "nae_denoise_block_f32, time_smooth 8, freq_smooth 4", lambda: ctx.denoise_block(gate, d_prof.ptr, ch, src, T, ch, n_streams, dst))]
        for mask in nae.HPSS_MASKS:
            p = nae.Context.hpss_design(0.0, -120.0, n_fft, 8, 8, mask)
            cases.append((f"K21 {mask}", f"nae_hpss_block_f32, spans 8, {mask} mask", lambda p=p: ctx.hpss_block(p, src, T, ch, n_streams, dst)))
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        samples = n_streams * ch * T
        base = statistics.median(ms["K13"])
        rows = []
        for tag, what, _ in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "n_fft": n_fft, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "gbytes_per_s": samples * 8 / med / 1e6, "ratio_to_k13": med / base})
            print(f"{name}, n_fft {n_fft}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); "
                  f"{samples * 8 / med / 1e6:.1f} GB/s; {med / base:.2f} x K13", flush=True)
        nodetime.release(d_in, d_out, d_prof)
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": [clock_before, clock_after], "rows": rows}), flush=True)


def main():
    ap = nodetime.parser(180.0, "a sixteenth of the streams, and a fifth of the length", step="--n-fft", what="frame size", type=int)
    ap.add_argument("--sizes", default="512,1024,2048,4096", help="the frame sizes, comma separated")
    args = ap.parse_args()
    if args.n_fft:
        run_size(args.n_fft, args.quick, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick, args.sizes), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
