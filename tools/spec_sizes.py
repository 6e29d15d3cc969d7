#!/usr/bin/env python3
"""K8 spectrum at every size on a chip-filling shape: 256 interleaved-stereo streams x 480 000 sample-frames (the C5 rank-of-4
size), hop = n_fft/4.  Per size one JSON line: kernel time from hipEvent pairs around each launch (nae_prof_*, after warm-up),
algorithmic bytes (input once + magnitudes out), those bytes / time as a fraction of 8 TB/s, time / byte floor at 8 TB/s, and the
shader clock (nae_debug_clock_ghz) right after the timed launches.  --sizes 256,4096 --reps 10 --streams 256 --frames 480000.
--layout interleaved (default) | planar (stereo) | mono; --generic 1: debug key spec_generic (interleaved stereo through the
generic 1024-point kernel).  The A/B of a change to the 1024-point kernels: --sizes 1024 --streams 1024 per layout, one line each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=480000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spec-any", type=int, default=0, help="1: the 1024-point line runs the size-generic kernel too")
    ap.add_argument("--layout", choices=["interleaved", "planar", "mono"], default="interleaved")
    ap.add_argument("--generic", type=int, default=0, help="1: debug key spec_generic (no interleaved-stereo fast path)")
    a = ap.parse_args()
    nae = naeload.load()
    ctx = nae.Context(0)
    S, n = a.frames, a.streams
    ch = 1 if a.layout == "mono" else 2
    d_x = ctx.empty(n * S * ch)
    ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n, 0, 0)
    src = nae.Sig.interleaved(d_x.ptr, S, ch) if a.layout == "interleaved" else nae.Sig.planar(d_x.ptr, S, ch)
    if a.spec_any:
        ctx.debug_set("spec_any", 1)
    if a.generic:
        ctx.debug_set("spec_generic", 1)
    for n_fft in [int(v) for v in a.sizes.split(",")]:
        hop, B = n_fft // 4, n_fft // 2 + 1
        F = ctx.spectrum_frames_ex(S, n_fft, hop)
        d_o = ctx.empty(n * F * ch * B)
        run = lambda: ctx.spectrum_block_ex(n_fft, hop, src, S, ch, n, d_o.ptr, F * ch * B)
        for _ in range(a.warmup):
            run()
        ctx.sync()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            run()
        ctx.sync()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        ghz = ctx.clock_ghz()
        total = sum(v[0] for v in rep.values())
        launches = max(v[1] for v in rep.values())
        ms = total / launches
        nbytes = n * S * ch * 4 + n * F * ch * B * 4
        floor_ms = nbytes / HBM_PEAK * 1e3
        print(json.dumps({"n_fft": n_fft, "hop": hop, "layout": a.layout, "generic": a.generic, "streams": n, "frames_per_stream": F,
                          "kernels": sorted(rep),
                          "ms": round(ms, 4), "bytes": nbytes, "frac_of_8TBps": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                          "x_floor": round(ms / floor_ms, 3), "clock_ghz": round(ghz, 3)}), flush=True)
        d_o.free()
    d_x.free()
    ctx.close()


if __name__ == "__main__":
    main()
