#!/usr/bin/env python3
"""Locked against unlocked K7 vocoder (NAE_STRETCH_PHASE_LOCK), timed interleaved in one process: per shape and repetition the unlocked
and the locked block call run back to back, and the vocoder's kernel times come from hipEvent pairs around each launch (nae_prof_*,
after warm-up).  The transposer's launches are left out (they are the same in both modes).  Shapes (--shapes, comma separated):
  c5   1024 streams x 10 s of stereo at 48 kHz, +3 semitones (BASELINE's C5 batch)
  c3   one stream of one hour of stereo, +3 semitones (C3)
  s16  16 streams x 60 s of stereo, +3 semitones
One JSON line per shape: median ms of the unlocked and the locked vocoder kernels, their ratio, and the per-kernel medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402

SHAPES = {"c5": (1024, 480_000), "c3": (1, 3600 * 48_000), "s16": (16, 60 * 48_000)}
PV_KERNELS = ("pv_", "pvlock_")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5,c3,s16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--semitones", type=float, default=3.0)
    a = ap.parse_args()
    nae = naeload.load()
    pitch = 2 ** (a.semitones / 12)
    for shape in a.shapes.split(","):
        n, S = SHAPES[shape]
        ch = 2
        with nae.Context(0) as ctx:
            pl = ctx.stretch_plan(1.0, pitch, S)
            d_x, d_o = ctx.empty(n * S * ch), ctx.empty(n * pl.out_len * ch)
            ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n, 0, 0)
            src, dst = nae.Sig.interleaved(d_x.ptr, S, ch), nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)

            def timed(lock):
                ctx.prof_reset()
                ctx.prof_enable(True)
                ctx.stretch_block(1.0, pitch, src, S, ch, n, dst, phase_lock=lock)
                ctx.sync()
                rep = ctx.prof_report()
                ctx.prof_enable(False)
                return {k: v[0] for k, v in rep.items() if k.startswith(PV_KERNELS)}

            for _ in range(a.warmup):
                timed(False), timed(True)
            runs = {False: [], True: []}
            for _ in range(a.reps):
                for lock in (False, True):
                    runs[lock].append(timed(lock))
            out = {"shape": shape, "streams": n, "frames_per_stream": S, "pitch": pitch}
            for lock, key in ((False, "unlocked"), (True, "locked")):
                tot = [sum(r.values()) for r in runs[lock]]
                out[key + "_ms"] = float(np.median(tot))
                out[key + "_kernels_ms"] = {k: float(np.median([r.get(k, 0.0) for r in runs[lock]])) for k in runs[lock][0]}
            out["ratio"] = out["locked_ms"] / out["unlocked_ms"]
            out["clock_ghz"] = ctx.clock_ghz()
            print(json.dumps(out), flush=True)
            d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
