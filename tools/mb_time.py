#!/usr/bin/env python3
"""Times nae_mb_block_f32 (K20, the multiband compressor) at two, three and four bands, without look-ahead and with the longest, next to the
composition of existing entries it replaces — B x nae_eq_block_f32 on the sections of every band's path plus B x nae_dyn_block_f32 — and
nae_gain_sig_f32, between two nae_event_records: warm, interleaved (every round times every case once, in turn), the median over the
rounds, with the shader clock read before and after.  A second pass under the library's per-kernel profile gives every kernel's share: the
median over the rounds of each kernel's total per call.

    python tools/mb_time.py [--runs 5] [--warmup 2] [--quick] [--limit SECONDS]

Cases, stereo at 48 kHz, linked, on uniform noise of +-1 whose level swells every 0.25 s between -54 and -6 dB (crossovers 200 | 120, 2500 |
120, 1000, 6000 Hz; every band threshold -30 dB, ratio 4, knee 6 dB, attack 5 ms, release 100 ms):
  g            nae_gain_sig_f32: 16 bytes per stereo frame
  M2 M3 M4     nae_mb_block_f32 at look-ahead 0;  M2L M3L M4L at look-ahead 1024
  C2 C3 C4     the composition at look-ahead 0;   C2L C3L C4L at look-ahead 1024 (its sum is not computed: it is charged nothing for it)
Beside each case the HBM floor (16 bytes per frame over 6.29 TB/s) is printed.
Shapes: 1024 stereo streams x 10 s (--quick: 64 streams x 2 s).  Every shape is a step of nodetime.drive under --limit (default 400 s).  One
JSON line per shape.
Steps: large (--quick: quick-large)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000), "quick-large": ("64 streams x 2 s", 64, 96000)}
HBM_BYTES_PER_S = 6.29e12
RATE = 48000
CROSSOVERS = {2: (200.0,), 3: (120.0, 2500.0), 4: (120.0, 1000.0, 6000.0)}
PATHS = {2: ((0, 1), (2, 3)), 3: ((0, 1, 2), (3, 4, 5, 6), (3, 4, 7, 8)), 4: ((0, 1, 2, 3, 4), (0, 1, 2, 5, 6), (7, 8, 9, 10, 11), (7, 8, 9, 12, 13))}


def steps(quick):
    return nodetime.shape_steps(quick, ("large",))


def run_shape(shape, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = SHAPES[shape]
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

        def composition(p, n_bands, band):
            coef = np.array([[p.coef[s][i] for i in range(5)] for s in range(p.n_sections)])
            for b in range(n_bands):
                ctx.eq_block(coef[list(PATHS[n_bands][b])], src, T, ch, n_streams, dst)
                ctx.dyn_block(band, dst, T, ch, n_streams, dst)

        for la in (0, 1024):
            tail = "L" if la else ""
            for n_bands in (2, 3, 4):
                band = nae.Context.dyn_design(RATE, threshold_db=-30.0, lookahead_s=la / RATE)
                p = nae.Context.mb_design(RATE, CROSSOVERS[n_bands], [band] * n_bands)
                cases.append((f"M{n_bands}{tail}", f"nae_mb_block_f32, {n_bands} bands, look-ahead {la}", lambda p=p: ctx.mb_block(p, src, T, ch, n_streams, dst)))
                cases.append((f"C{n_bands}{tail}", f"{n_bands} x eq + {n_bands} x dyn, look-ahead {la}",
                              lambda p=p, n_bands=n_bands, band=band: composition(p, n_bands, band)))
        ms, clock_before, clock_after = nodetime.rounds(ctx, cases, runs, warmup)
        # every kernel's total per call, under the profile (an event pair around every launch)
        kernels = {c[0]: {} for c in cases}
        ctx.prof_enable(True)
        for _ in range(runs):
            for tag, _, fn in cases:
                ctx.prof_reset()
                fn()
                ctx.sync()
                for kernel, (total_ms, launches) in ctx.prof_report().items():
                    kernels[tag].setdefault(kernel, []).append((total_ms, launches))
        ctx.prof_enable(False)
        clock_last = ctx.clock_ghz()
        floor_ms = traffic / HBM_BYTES_PER_S * 1e3
        rows = []
        for tag, what, _ in cases:
            med = statistics.median(ms[tag])
            per_kernel = {k: {"ms": statistics.median(t for t, _ in v), "launches": int(v[0][1])} for k, v in kernels[tag].items()}
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]), "bytes": traffic,
                         "gbytes_per_s": traffic / med / 1e6, "hbm_floor_ms": floor_ms, "kernels": per_kernel})
            shares = "; ".join(f"{k} {v['ms']:.3f} ms in {v['launches']}" for k, v in sorted(per_kernel.items()))
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {med / floor_ms:.2f} x the HBM floor of "
                  f"{floor_ms:.3f} ms; kernels: {shares}", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: " + ", ".join(f"M{k}/C{k} {t[f'M{k}'] / t[f'C{k}']:.3f}" for k in ("2", "3", "4", "2L", "3L", "4L")) +
              f"; clock {clock_before:.3f} GHz before, {clock_after:.3f} GHz after the timed rounds, {clock_last:.3f} GHz after the profiled ones", flush=True)
        nodetime.release(d_in, d_out)
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": [clock_before, clock_after, clock_last], "rows": rows}), flush=True)


def main():
    args = nodetime.parser(400.0, runs=5, choices=sorted(SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
