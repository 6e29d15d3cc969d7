#!/usr/bin/env python3
"""Formant preservation's cost (nae_stretch_block_formant_f32 against the same call without a lifter), timed interleaved in one process: per
frame size and repetition the call runs with lifter 0 and with the default lifter back to back, and the kernel times come from hipEvent pairs
around each launch (nae_prof_*, after warm-up).  Default shape: 256 streams x 10 s of stereo at 48 kHz, pitch +4 semitones (the transposer
first); --locked adds 1024 with NAE_STRETCH_PHASE_LOCK.
One JSON line per size: median ms of the synthesis pass (pass 3: the *synth* kernels, and at 1024 unflagged the vocoder pipeline's pv_pipe /
pv_flow kernels) and of every kernel of the call, off and on, and their ratios."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

PASS3 = ("pv_pipe", "pv_flow")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--semitones", type=float, default=4.0)
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--locked", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    nae = naeload.load()
    n_streams, S, ch = a.streams, int(a.seconds * 48000), 2
    rate, pitch = 1.0, 2 ** (a.semitones / 12)
    keys = [(int(n), False) for n in a.sizes.split(",")] + ([(1024, True)] if a.locked else [])
    with nae.Context(0) as ctx:
        out_len = max(ctx.stretch_plan(rate, pitch, S, n).out_len for n, _ in keys)
        d_x, d_o = ctx.empty(n_streams * S * ch), ctx.empty(n_streams * out_len * ch)
        ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n_streams, 0, 0)
        src = nae.Sig.interleaved(d_x.ptr, S, ch)

        def timed(n_fft, lock, lifter):
            pl = ctx.stretch_plan(rate, pitch, S, n_fft)
            ctx.prof_reset()
            ctx.prof_enable(True)
            ctx.stretch_block(rate, pitch, src, S, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch), phase_lock=lock, n_fft=n_fft,
                              formant=lifter)
            ctx.sync()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            return {k: v[0] for k, v in rep.items()}

        for n_fft, lock in keys:
            q = nae.formant_lifter(48000, n_fft)
            for _ in range(a.warmup):
                timed(n_fft, lock, 0), timed(n_fft, lock, q)
            runs = {0: [], q: []}
            for _ in range(a.reps):
                for lifter in (0, q):
                    runs[lifter].append(timed(n_fft, lock, lifter))
            out = {"n_fft": n_fft, "locked": lock, "lifter": q, "streams": n_streams, "frames_per_stream": S, "semitones": a.semitones}
            for lifter, tag in ((0, "off"), (q, "on")):
                synth = float(np.median([sum(v for k, v in r.items() if "synth" in k or k.startswith(PASS3)) for r in runs[lifter]]))
                total = float(np.median([sum(r.values()) for r in runs[lifter]]))
                out[tag] = {"synth_ms": synth, "call_kernels_ms": total,
                            "kernels_ms": {k: float(np.median([r.get(k, 0.0) for r in runs[lifter]])) for k in runs[lifter][0]}}
            out["synth_ratio"] = out["on"]["synth_ms"] / out["off"]["synth_ms"]
            out["call_ratio"] = out["on"]["call_kernels_ms"] / out["off"]["call_kernels_ms"]
            out["clock_ghz"] = ctx.clock_ghz()
            print(json.dumps(out), flush=True)
        d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
