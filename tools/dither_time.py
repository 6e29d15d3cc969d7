#!/usr/bin/env python3
"""Times nae_dither_block_f32 (K23, the dither) without taps next to nae_gain_sig_f32 at the same bytes, and with 1, 5 and 12 taps, between
two nae_event_records: warm, interleaved (every round times every case once, in turn), the median over the rounds, with the shader clock
read before and after.

    python tools/dither_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz, 16 bits, triangular dither, on uniform noise of +-1:
  g     nae_gain_sig_f32: 16 bytes per stereo frame
  f     the dither without taps (dither_flat_kernel): the same bytes
  fh    the same with the highpass dither (a second hash per sample)
  K1    error feedback with the `first` preset           (dither_ef_kernel<1>, producer waves)
  K5    ... with the `lipshitz` preset                   (dither_ef_kernel<5>, producer waves)
  K12   ... with 12 drawn taps                           (dither_ef_kernel<12>, producer waves)
  K5w   K5 with the feed-forward work in the walking wave (debug key dither_roles = 2): what the roles buy
Beside each case the HBM floor (16 bytes per frame over 6.29 TB/s) is printed, and for the error-feedback cases the nanoseconds per sample
of one stream-channel (the time is proportional to the length, and nearly independent of the batch until the batch fills the SIMDs);
the ratios f/g and K5w/K5 are reported, nothing is asserted about them.
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s (--quick: 64 streams x 2 s and 8 streams x 2 s), each a step of
nodetime.drive under --limit (default 240 s).  One JSON line per shape.
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps
HBM_BYTES_PER_S = 6.29e12
DRAWN = (0.41, -0.37, 0.29, -0.33, 0.21, 0.27, -0.19, 0.23, -0.17, 0.13, -0.22, 0.18)   # 12 taps of absolute sum 3


def run_shape(shape, runs, warmup):
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        traffic = 2 * n_streams * ch * T * 4

        def dither(p, roles=0):
            def call():
                if roles:
                    ctx.debug_set("dither_roles", roles)
                ctx.dither_block(p, src, T, ch, n_streams, dst)
                if roles:
                    ctx.debug_set("dither_roles", 0)
            return call
        p12 = nae.dither_design(16, "triangular", "none")
        p12.n_taps = 12
        for k, c in enumerate(DRAWN):
            p12.taps[k] = c
        cases = [("g", "nae_gain_sig_f32", lambda: ctx.gain_sig(src, dst, T, ch, n_streams, 0.5)),
                 ("f", "dither without taps, triangular", dither(nae.dither_design(16, "triangular", "none"))),
                 ("fh", "dither without taps, highpass", dither(nae.dither_design(16, "highpass", "none"))),
                 ("K1", "error feedback, 1 tap", dither(nae.dither_design(16, "triangular", "first"))),
                 ("K5", "error feedback, 5 taps", dither(nae.dither_design(16, "triangular", "lipshitz"))),
                 ("K12", "error feedback, 12 taps", dither(p12)),
                 ("K5w", "error feedback, 5 taps, all work in the walking wave", dither(nae.dither_design(16, "triangular", "lipshitz"), roles=2))]
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        floor_ms = traffic / HBM_BYTES_PER_S * 1e3
        rows = []
        for tag, what, _ in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]), "bytes": traffic,
                         "gbytes_per_s": traffic / med / 1e6, "hbm_floor_ms": floor_ms, "ns_per_sample": med * 1e6 / T})
            per = f"; {med * 1e6 / T:.2f} ns per sample of a stream-channel" if tag.startswith("K") else ""
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s; "
                  f"{med / floor_ms:.2f} x the HBM floor of {floor_ms:.3f} ms{per}", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: f/g {t['f'] / t['g']:.3f}, fh/g {t['fh'] / t['g']:.3f}, K5w/K5 {t['K5w'] / t['K5']:.3f}; clock {clock_before:.3f} GHz before, "
              f"{clock_after:.3f} GHz after", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": [clock_before, clock_after], "rows": rows}), flush=True)


def main():
    args = nodetime.parser(240.0, choices=sorted(nodetime.SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
