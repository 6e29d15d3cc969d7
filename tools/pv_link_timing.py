#!/usr/bin/env python3
"""The channel link's cost (NAE_STRETCH_LINK_CHANNELS against the same flagged call without it), timed interleaved in one process: per route
and repetition the block call runs unlinked and linked back to back — every frame size with NAE_STRETCH_TRANSIENTS, and with --locked 1024
with NAE_STRETCH_PHASE_LOCK and with both — and the kernel times come from hipEvent pairs around each launch (nae_prof_*, after warm-up).
Shapes: --streams stereo streams of --seconds at 48 kHz, velocity 1.5 with keep_pitch (no transposer; uniform noise, which has no onsets).
One JSON line per route: median ms of pass 1 (the *phase* / pvlock_map kernels), pass 2 (the *scan* kernels) and pass 3 (the *synth*
kernels), off (unlinked) and on (linked), and their ratios."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

PASSES = {"pass1": lambda k: "phase" in k or "map" in k, "pass2": lambda k: "scan" in k, "pass3": lambda k: "synth" in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--locked", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    nae = naeload.load()
    n_streams, S, ch = a.streams, int(a.seconds * 48000), 2
    rate, pitch = 1.5, 1 / 1.5
    sizes = [int(n) for n in a.sizes.split(",")]
    with nae.Context(0) as ctx:
        out_len = max(ctx.stretch_plan(rate, pitch, S, n).out_len for n in sizes)
        d_x, d_o = ctx.empty(n_streams * S * ch), ctx.empty(n_streams * out_len * ch)
        ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n_streams, 0, 0)
        src = nae.Sig.interleaved(d_x.ptr, S, ch)

        def timed(n_fft, link, lock, transients):
            pl = ctx.stretch_plan(rate, pitch, S, n_fft)
            ctx.prof_reset()
            ctx.prof_enable(True)
            ctx.stretch_block(rate, pitch, src, S, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch), n_fft=n_fft,
                              transients=transients, phase_lock=lock, link_channels=link)
            ctx.sync()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            return {k: v[0] for k, v in rep.items()}

        jobs = [(n_fft, "transients", False, True) for n_fft in sizes]
        jobs += [(1024, "locked", True, False), (1024, "locked+transients", True, True)] if a.locked else []
        for n_fft, route, lock, tr in jobs:
            for _ in range(a.warmup):
                timed(n_fft, False, lock, tr), timed(n_fft, True, lock, tr)
            runs = {False: [], True: []}
            for _ in range(a.reps):
                runs[False].append(timed(n_fft, False, lock, tr))
                runs[True].append(timed(n_fft, True, lock, tr))
            out = {"n_fft": n_fft, "route": route, "streams": n_streams, "seconds": a.seconds}
            for lk, tag in ((False, "off"), (True, "on")):
                out[tag] = {p: float(np.median([sum(v for k, v in r.items() if f(k)) for r in runs[lk]])) for p, f in PASSES.items()}
                out[tag]["call"] = float(np.median([sum(r.values()) for r in runs[lk]]))
                out[tag]["kernels_ms"] = {k: float(np.median([r.get(k, 0.0) for r in runs[lk]])) for k in runs[lk][0]}
            out["ratio"] = {p: (out["on"][p] / out["off"][p] if out["off"][p] > 0 else None) for p in list(PASSES) + ["call"]}
            out["clock_ghz"] = ctx.clock_ghz()
            print(json.dumps(out), flush=True)
        d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
