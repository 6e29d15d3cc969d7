#!/usr/bin/env python3
"""Times nae_denoise_block_f32 (K13, the spectral gate) between two nae_event_records next to the formant shift's envelope pass
(pv_env_kernel: nae_stretch_block_formant_shift_f32 at tempo and pitch 1) at the same frame size and shape, the two calls alternating in one
process: warm, the median of several runs.

    python tools/denoise_time.py [--runs 7] [--warmup 2] [--quick] [--limit SECONDS] [--n-fft 2048]

Shapes: 1024 stereo streams x 10 s at 48 kHz with the library's tile, and 8 stereo streams x 60 s with the library's tile and with forced ones
(debug key dn_tile) (--quick: 64 streams x 2 s and 8 streams x 6 s).  The node's defaults: 12 dB reduction, 6 dB sensitivity, Tn = Fn = 2;
the profile is learned from the first half second of stream 0.  Every shape is a step of nodetime.drive under --limit (default 180 s).  Per
case: the time and the traffic rate at the 8 bytes per sample and channel the call must move.  One JSON line per shape
(profiles/r19_denoise.md is written from them).
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps
SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000, (0,)), "small": ("8 streams x 60 s", 8, 2880000, (0, 8, 16, 32, 128, 512)),
          "quick-large": ("64 streams x 2 s", 64, 96000, (0,)), "quick-small": ("8 streams x 6 s", 8, 288000, (0, 8, 16, 32, 128, 512))}


def run_shape(key, runs, warmup, n_fft):
    import statistics
    import naeload
    nae = naeload.load()
    name, n_streams, T, tiles = SHAPES[key]
    rows, ch = [], 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        d_prof = ctx.empty(ch * (n_fft // 2 + 1))
        ctx.denoise_profile(n_fft, src, 24000, ch, d_prof.ptr)
        p = nae.Context.denoise_design(12.0, 6.0, n_fft, 2, 2)
        q, phi = nae.formant_lifter(48000, n_fft), 2 ** (4 / 12)
        assert ctx.stretch_plan(1.0, 1.0, T, n_fft, formant=q, formant_ratio=phi).out_len == T
        cases = [("env", "env", lambda: ctx.stretch_block(1.0, 1.0, src, T, ch, n_streams, dst, n_fft=n_fft, formant=q, formant_ratio=phi))]
        for tile in tiles:
            def gate(tile=tile):
                ctx.debug_set("dn_tile", tile)
                ctx.denoise_block(p, d_prof.ptr, ch, src, T, ch, n_streams, dst)
            cases.append((f"gate, dn_tile {tile}", "gate", gate))
        ms, _, _ = nodetime.rounds(ctx, cases, runs, warmup, clock=False)    # alternating: every round times every call once
        samples = n_streams * ch * T
        for k, v in ms.items():
            med = statistics.median(v)
            rows.append({"shape": name, "n_fft": n_fft, "call": k, "ms": med, "min_ms": min(v), "max_ms": max(v), "gbytes_per_s": samples * 8 / med / 1e6,
                         "ratio_to_env": med / statistics.median(ms["env"])})
            print(f"{name}, n_fft {n_fft}: {k}: {med:.3f} ms (min {min(v):.3f}, max {max(v):.3f}); {samples * 8 / med / 1e6:.1f} GB/s; "
                  f"{med / statistics.median(ms['env']):.2f}x the envelope pass", flush=True)
        ghz = ctx.clock_ghz()
        nodetime.release(d_in, d_out, d_prof)
        print(json.dumps({"device": ctx.name(), "runs": runs, "clock_ghz": ghz, "rows": rows}), flush=True)


def main():
    ap = nodetime.parser(180.0, "a sixteenth of the large shape's streams, and a fifth or a tenth of the lengths", choices=sorted(SHAPES))
    ap.add_argument("--n-fft", type=int, default=2048)
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup, args.n_fft)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args) + ["--n-fft", str(args.n_fft)])


if __name__ == "__main__":
    sys.exit(main())
