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
Shapes: 1024 stereo streams x 10 s and 8 stereo streams x 10 s at 48 kHz (--quick: 64 streams x 2 s and 8 streams x 2 s).  Every shape is a step of
nodetime.drive under --limit (default 180 s).  Traffic is counted at 4 bytes per sample read or written once: the signal in and out, and
the key where it is another signal.  One JSON line per shape (profiles/r21_dynkey.md is written from them).
Steps: large, small (--quick: quick-large, quick-small)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nodetime  # noqa: E402

steps = nodetime.shape_steps


def run_shape(shape, runs, warmup):
    import numpy as np
    import naeload
    nae = naeload.load()
    name, n_streams, T = nodetime.SHAPES[shape]
    ch = 2
    with nae.Context(0) as ctx:
        d_in, d_out, src, dst = nodetime.setup(nae, ctx, n_streams, T)
        d_key, d_scratch = ctx.empty(n_streams * T * ch), ctx.empty(n_streams * T * ch)
        ctx.fill_uniform(d_key.ptr, T * ch, T * ch, n_streams, 0, 1)
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
        ms, _, _ = nodetime.rounds(ctx, cases, runs, warmup, clock=False)
        rows = []
        for tag, what, _, traffic in cases:
            med = statistics.median(ms[tag])
            rows.append({"shape": name, "case": tag, "what": what, "ms": med, "min_ms": min(ms[tag]), "max_ms": max(ms[tag]),
                         "bytes": traffic, "gbytes_per_s": traffic / med / 1e6})
            print(f"{name}: ({tag}) {what}: {med:.3f} ms (min {min(ms[tag]):.3f}, max {max(ms[tag]):.3f}); {traffic / med / 1e6:.1f} GB/s", flush=True)
        t = {r["case"]: r["ms"] for r in rows}
        print(f"{name}: b/a {t['b'] / t['a']:.3f} (traffic 3/2), c/a {t['c'] / t['a']:.3f}, d/a {t['d'] / t['a']:.3f}, d/e {t['d'] / t['e']:.3f}", flush=True)
        nodetime.release(d_in, d_out, d_key, d_scratch)
        print(json.dumps({"device": ctx.name(), "runs": runs, "rows": rows}), flush=True)


def main():
    args = nodetime.parser(180.0, choices=sorted(nodetime.SHAPES)).parse_args()
    if args.shape:
        run_shape(args.shape, args.runs, args.warmup)
        return 0
    return nodetime.drive(__file__, steps(args.quick), args.limit, nodetime.counts(args))


if __name__ == "__main__":
    sys.exit(main())
