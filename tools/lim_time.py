#!/usr/bin/env python3
"""Times nae_lim_block_f32 (K22, the limiter) with the true-peak detector and with the sample-peak detector next to nae_dyn_block_f32 (K12) in
limiter mode at the same look-ahead and nae_gain_sig_f32, between two nae_event_records: warm, interleaved (every round times every case
once, in turn), the median over the rounds, with the shader clock read before and after.

    python tools/lim_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz, linked, on uniform noise of +-1 whose level swells every 0.25 s between -30 and +18 dB around -6 dB, so a limiter
at -1 dB works and rests (look-ahead 72 samples, release 100 ms):
  g    nae_gain_sig_f32: 16 bytes per stereo frame
  d72  nae_dyn_block_f32 in limiter mode (threshold -1 dB, ratio inf, no knee, attack 0, release 100 ms) at look-ahead 72
  T72  the limiter with true_peak = 1 at look-ahead 72 (ceiling -1 dB, gain 0 dB)
  S72  the limiter with true_peak = 0 at look-ahead 72
Beside each case the HBM floor (16 bytes per frame over 6.29 TB/s) is printed; the ratios T72/d72 and S72/d72 are reported, nothing is
asserted about them.
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
RATE = 48000


def run_shape(shape, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        # the swell: one stream's envelope, applied in place to every stream by the library's own gain, 0.25 s at a time
        for k in range(T // (RATE // 4)):
            level = 10.0 ** ((-6.0 + 24.0 * np.sin(2 * np.pi * k / 7.0)) / 20.0)
            part = nae.Sig(d_in.at(k * (RATE // 4) * ch), T * ch, 1, ch)
            ctx.gain_sig(part, part, RATE // 4, ch, n_streams, float(level))
        traffic = 2 * n_streams * ch * T * 4
        cases = [("g", "nae_gain_sig_f32", lambda: ctx.gain_sig(src, dst, T, ch, n_streams, 0.5))]
        LA = 72
        p = nae.Context.dyn_design(RATE, threshold_db=-1.0, ratio=float("inf"), knee_db=0.0, attack_s=0.0, release_s=0.1, lookahead_s=LA / RATE)
        cases.append((f"d{LA}", f"nae_dyn_block_f32 in limiter mode, look-ahead {LA}", lambda p=p: ctx.dyn_block(p, src, T, ch, n_streams, dst)))
        for tag, tp in (("T", True), ("S", False)):
            p = nae.Context.lim_design(RATE, ceiling_db=-1.0, gain_db=0.0, release_s=0.1, lookahead_s=LA / RATE, true_peak=tp)
            cases.append((f"{tag}{LA}", f"limiter, true_peak {int(tp)}, look-ahead {LA}", lambda p=p: ctx.lim_block(p, src, T, ch, n_streams, dst)))
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        floor_ms = traffic / HBM_BYTES_PER_S * 1e3
        rows = []
        for tag, what, _ in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]), "bytes": traffic,
                         "gbytes_per_s": traffic / med / 1e6, "hbm_floor_ms": floor_ms})
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s; "
                  f"{med / floor_ms:.2f} x the HBM floor of {floor_ms:.3f} ms", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: T72/d72 {t['T72'] / t['d72']:.3f}, S72/d72 {t['S72'] / t['d72']:.3f}; clock {clock_before:.3f} GHz before, {clock_after:.3f} GHz after",
              flush=True)
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
