#!/usr/bin/env python3
"""Times nae_sat_block_f32 (K18, the saturation) at every oversampling factor and curve next to nae_eq_block_f32 and nae_gain_sig_f32, between
two nae_event_records: warm, interleaved (every round times every case once, in turn), the median over the rounds, with the shader clock read
before and after.

    python tools/sat_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS] [--tile N]

Cases, stereo at 48 kHz, drive 12 dB on uniform noise of +-1, bias 0, wet 1, dry 0:
  g        nae_gain_sig_f32: 16 bytes per stereo frame
  q        nae_eq_block_f32, two sections (a low-pass and a high-pass)
  s1 ... s8 / h1 ... h8   the soft and the hard curve at oversample 1, 2, 4 and 8
Beside each case the HBM floor (16 bytes per frame over 6.29 TB/s) is printed; the VALU floor is worked out in profiles/r26_sat.md from the
v_* instructions of the two loop bodies in the gfx950 ISA (hipcc -S), at 2.15 cycles per wave-instruction and the clock printed here.  --tile forces sat_tile (chunks per wave).
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


def run_shape(shape, runs, warmup, tile):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        if tile:
            ctx.debug_set("sat_tile", tile)
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        coef = np.stack([nae.Context.eq_design("lowpass", 48000, 4000.0), nae.Context.eq_design("highpass", 48000, 100.0)])
        traffic = 2 * n_streams * ch * T * 4
        cases = [("g", "nae_gain_sig_f32", lambda: ctx.gain_sig(src, dst, T, ch, n_streams, 0.5)),
                 ("q", "nae_eq_block_f32, 2 sections", lambda: ctx.eq_block(coef, src, T, ch, n_streams, dst))]
        for curve in ("soft", "hard"):
            for m in (1, 2, 4, 8):
                p = nae.Context.sat_design(12.0, 0.0, curve, m)
                cases.append((f"{curve[0]}{m}", f"saturation, {curve}, oversample {m}", lambda p=p: ctx.sat_block(p, src, T, ch, n_streams, dst)))
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
        print(f"{name}: s1/g {t['s1'] / t['g']:.3f}, h1/g {t['h1'] / t['g']:.3f}, s4/q {t['s4'] / t['q']:.3f}; sat_tile {tile}; "
              f"clock {clock_before:.3f} GHz before, {clock_after:.3f} GHz after", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "sat_tile": tile, "clock_ghz": [clock_before, clock_after], "rows": rows}), flush=True)


def main():
    ap = nodetime.parser(240.0, choices=sorted(nodetime.SHAPES))
    ap.add_argument("--tile", type=int, default=0, help="sat_tile: chunks per wave (0: the library's pick)")
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup, args.tile)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args) + ["--tile", str(args.tile)])


if __name__ == "__main__":
    sys.exit(main())
