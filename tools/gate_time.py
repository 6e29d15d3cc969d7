#!/usr/bin/env python3
"""Times nae_gate_block_f32 (K19, the gate) in both modes, without look-ahead and with the longest, next to nae_dyn_block_f32 (K12) and
nae_gain_sig_f32, between two nae_event_records: warm, interleaved (every round times every case once, in turn), the median over the
rounds, with the shader clock read before and after.

    python tools/gate_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz, linked, on uniform noise of +-1 whose level swells every 0.25 s between -54 and -6 dB, so a gate at -30 dB opens
and closes (threshold -30 dB, hysteresis 3 dB, range 60 dB, ratio 2, attack 1 ms, hold 50 ms, release 100 ms):
  g          nae_gain_sig_f32: 16 bytes per stereo frame
  d0, d1024  nae_dyn_block_f32 (threshold -18 dB, ratio 4, knee 6 dB, attack 5 ms, release 100 ms) at look-ahead 0 and 1024
  G0, G1024  the gate mode at look-ahead 0 and 1024
  E0, E1024  the expander mode at look-ahead 0 and 1024
Beside each case the HBM floor (16 bytes per frame over 6.29 TB/s) is printed.
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a step of
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
            level = 10.0 ** ((-30.0 + 24.0 * np.sin(2 * np.pi * k / 7.0)) / 20.0)
            part = nae.Sig(d_in.at(k * (RATE // 4) * ch), T * ch, 1, ch)
            ctx.gain_sig(part, part, RATE // 4, ch, n_streams, float(level))
        traffic = 2 * n_streams * ch * T * 4
        cases = [("g", "nae_gain_sig_f32", lambda: ctx.gain_sig(src, dst, T, ch, n_streams, 0.5))]
        for la in (0, 1024):
            p = nae.Context.dyn_design(RATE, lookahead_s=la / RATE)
            cases.append((f"d{la}", f"nae_dyn_block_f32, look-ahead {la}", lambda p=p: ctx.dyn_block(p, src, T, ch, n_streams, dst)))
        for mode in nae.GATE_MODES:
            for la in (0, 1024):
                p = nae.Context.gate_design(RATE, mode, threshold_db=-30.0, lookahead_s=la / RATE)
                cases.append((f"{mode[0].upper()}{la}", f"gate, mode {mode}, look-ahead {la}", lambda p=p: ctx.gate_block(p, src, T, ch, n_streams, dst)))
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
        print(f"{name}: G0/d0 {t['G0'] / t['d0']:.3f}, G1024/d1024 {t['G1024'] / t['d1024']:.3f}, E0/d0 {t['E0'] / t['d0']:.3f}, "
              f"E1024/d1024 {t['E1024'] / t['d1024']:.3f}; clock {clock_before:.3f} GHz before, {clock_after:.3f} GHz after", flush=True)
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
