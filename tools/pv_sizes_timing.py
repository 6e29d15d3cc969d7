#!/usr/bin/env python3
"""The K7 vocoder at every frame size (nae_stretch_block_n_f32), timed interleaved in one process: per shape and repetition the block call runs
at 1024 (the shipped kernels) and at 512 / 2048 / 4096 (kernels_pv_any.hip) back to back, and the vocoder's kernel times come from hipEvent
pairs around each launch (nae_prof_*, after warm-up).  The transposer's launches are left out (they do not depend on the size).
Shapes (--shapes, comma separated):
  c5   1024 streams x 10 s of stereo at 48 kHz (BASELINE's C5 batch)
  c3   one stream of one hour of stereo (C3)
Parameters (--case): p3 = +3 semitones (rate 1, pitch 2^(3/12)); v15 = velocity 1.5 with keep_pitch (rate 1.5, pitch 1/1.5).
--pv-any also times 1024 through the size-generic kernels (debug key pv_any).
One JSON line per shape and case: median ms of the vocoder kernels per size, ns per input sample-frame, the ratio to 1024 and the per-kernel
medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

SHAPES = {"c5": (1024, 480_000), "c3": (1, 3600 * 48_000)}
CASES = {"p3": (1.0, 2 ** (3 / 12)), "v15": (1.5, 1 / 1.5)}
PV_KERNELS = ("pv_",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--cases", default="p3,v15")
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pv-any", action="store_true")
    a = ap.parse_args()
    nae = naeload.load()
    sizes = [int(v) for v in a.sizes.split(",")]
    keys = [(n, False) for n in sizes] + ([(1024, True)] if a.pv_any else [])
    for shape in a.shapes.split(","):
        n_streams, S = SHAPES[shape]
        ch = 2
        for case in a.cases.split(","):
            rate, pitch = CASES[case]
            with nae.Context(0) as ctx:
                out_len = max(ctx.stretch_plan(rate, pitch, S, n).out_len for n in sizes)
                d_x, d_o = ctx.empty(n_streams * S * ch), ctx.empty(n_streams * out_len * ch)
                ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n_streams, 0, 0)
                src = nae.Sig.interleaved(d_x.ptr, S, ch)

                def timed(key):
                    n_fft, generic = key
                    pl = ctx.stretch_plan(rate, pitch, S, n_fft)
                    ctx.debug_set("pv_any", 1 if generic else 0)
                    ctx.prof_reset()
                    ctx.prof_enable(True)
                    ctx.stretch_block(rate, pitch, src, S, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch), n_fft=n_fft)
                    ctx.sync()
                    rep = ctx.prof_report()
                    ctx.prof_enable(False)
                    return {k: v[0] for k, v in rep.items() if k.startswith(PV_KERNELS)}

                for _ in range(a.warmup):
                    for key in keys:
                        timed(key)
                runs = {key: [] for key in keys}
                for _ in range(a.reps):
                    for key in keys:
                        runs[key].append(timed(key))
                out = {"shape": shape, "case": case, "streams": n_streams, "frames_per_stream": S, "rate": rate, "pitch": pitch, "sizes": {}}
                for key in keys:
                    tot = float(np.median([sum(r.values()) for r in runs[key]]))
                    name = f"{key[0]}{'_pv_any' if key[1] else ''}"
                    out["sizes"][name] = {"ms": tot, "ns_per_frame": tot * 1e6 / (n_streams * S),
                                          "kernels_ms": {k: float(np.median([r.get(k, 0.0) for r in runs[key]])) for k in runs[key][0]}}
                base = out["sizes"]["1024"]["ms"] if "1024" in out["sizes"] else None
                if base:
                    for name, v in out["sizes"].items():
                        v["ratio_to_1024"] = v["ms"] / base
                out["clock_ghz"] = ctx.clock_ghz()
                print(json.dumps(out), flush=True)
                d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
