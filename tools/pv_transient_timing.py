#!/usr/bin/env python3
"""Transient preservation's cost (NAE_STRETCH_TRANSIENTS against the same call without it), timed interleaved in one process: per frame size
and repetition the block call runs unflagged and flagged back to back — at 1024 also unflagged on the size-generic kernels (debug key
pv_any = 1), the route the flagged call takes; --locked adds 1024 with NAE_STRETCH_PHASE_LOCK on both sides — and the kernel times come
from hipEvent pairs around each launch (nae_prof_*, after warm-up).
Shapes: --streams stereo streams of --seconds at 48 kHz, velocity 1.5 with keep_pitch (no transposer; uniform noise, which has no onsets).
One JSON line per size and route: median ms of pass 1 (the *phase* / pvlock_map kernels), pass 2 (the *scan* kernels) and pass 3 (the
*synth* kernels, and on the shipped 1024 route the vocoder pipeline's pv_pipe / pv_flow kernels), off and on, and their ratios."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

PASSES = {"pass1": lambda k: "phase" in k or "map" in k, "pass2": lambda k: "scan" in k,
          "pass3": lambda k: "synth" in k or k.startswith(("pv_pipe", "pv_flow"))}


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
    with nae.Context(0) as ctx, nae.Context(0) as gen:
        gen.debug_set("pv_any", 1)
        out_len = max(ctx.stretch_plan(rate, pitch, S, n).out_len for n in sizes)
        d_x, d_o = ctx.empty(n_streams * S * ch), ctx.empty(n_streams * out_len * ch)
        ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n_streams, 0, 0)
        src = nae.Sig.interleaved(d_x.ptr, S, ch)

        def timed(c, n_fft, transients, lock=False):
            pl = c.stretch_plan(rate, pitch, S, n_fft)
            c.prof_reset()
            c.prof_enable(True)
            c.stretch_block(rate, pitch, src, S, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch), n_fft=n_fft,
                            transients=transients, phase_lock=lock)
            c.sync()
            rep = c.prof_report()
            c.prof_enable(False)
            return {k: v[0] for k, v in rep.items()}

        jobs = []
        for n_fft in sizes:
            jobs += [(n_fft, "size-generic" if n_fft != 1024 else "shipped", ctx, False)]
            jobs += [(n_fft, "size-generic", gen, False)] if n_fft == 1024 else []
        jobs += [(1024, "locked", ctx, True)] if a.locked else []
        for n_fft, route, c_off, lock in jobs:
            for _ in range(a.warmup):
                timed(c_off, n_fft, False, lock), timed(ctx, n_fft, True, lock)
            runs = {False: [], True: []}
            for _ in range(a.reps):
                runs[False].append(timed(c_off, n_fft, False, lock))
                runs[True].append(timed(ctx, n_fft, True, lock))
            out = {"n_fft": n_fft, "off_route": route, "streams": n_streams, "seconds": a.seconds}
            for tr, tag in ((False, "off"), (True, "on")):
                out[tag] = {p: float(np.median([sum(v for k, v in r.items() if f(k)) for r in runs[tr]])) for p, f in PASSES.items()}
                out[tag]["call"] = float(np.median([sum(r.values()) for r in runs[tr]]))
                out[tag]["kernels_ms"] = {k: float(np.median([r.get(k, 0.0) for r in runs[tr]])) for k in runs[tr][0]}
            out["ratio"] = {p: (out["on"][p] / out["off"][p] if out["off"][p] > 0 else None) for p in list(PASSES) + ["call"]}
            out["clock_ghz"] = ctx.clock_ghz()
            print(json.dumps(out), flush=True)
        d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
