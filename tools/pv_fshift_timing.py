#!/usr/bin/env python3
"""The formant shift's envelope pass (pv_env_kernel: nae_stretch_block_formant_shift_f32 at pitch 1, the forced stage alone) next to the
formant pass 3 (pv_any_synth_formant_kernel: nae_stretch_block_formant_f32 at pitch 2^(1/12)), timed interleaved in one process: per frame size
and repetition the two calls run back to back, and the kernel times come from hipEvent pairs around each launch (nae_prof_*, after warm-up).
Default shape: 256 streams x 10 s of stereo at 48 kHz.  One JSON line per size: median, lowest and highest ms of each kernel, the frames each
walks per stream-channel (the plan's), ns per frame and stream-channel, and the ratio of the medians.  --kernel formant times the formant
pass 3 alone and uses nothing newer than nae_stretch_block_formant_f32, so the same file runs from a checkout of an older commit (copy it
into that tree's tools/): rounds of the two trees' runs, interleaved on one box, compare the parent's kernel with pv_env_kernel."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import naeload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--shift", type=float, default=4.0, help="formant shift of the envelope pass, semitones")
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel", choices=("both", "formant", "env"), default="both")
    a = ap.parse_args()
    nae = naeload.load()
    n_streams, S, ch = a.streams, int(a.seconds * 48000), 2
    phi, pitch = 2 ** (a.shift / 12), 2 ** (1 / 12)
    with nae.Context(0) as ctx:
        d_x, d_o = ctx.empty(n_streams * S * ch), ctx.empty(n_streams * S * ch)
        ctx.fill_uniform(d_x.ptr, S * ch, S * ch, n_streams, 0, 0)
        src = nae.Sig.interleaved(d_x.ptr, S, ch)

        def timed(n_fft, q, env):
            pl = ctx.stretch_plan(1.0, 1.0, S, n_fft, formant=q, formant_ratio=phi) if env else ctx.stretch_plan(1.0, pitch, S, n_fft)
            ctx.prof_reset()
            ctx.prof_enable(True)
            dst = nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)
            if env:
                ctx.stretch_block(1.0, 1.0, src, S, ch, n_streams, dst, n_fft=n_fft, formant=q, formant_ratio=phi)
            else:
                ctx.stretch_block(1.0, pitch, src, S, ch, n_streams, dst, n_fft=n_fft, formant=q)
            ctx.sync()
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            name = "pv_env_kernel" if env else "pv_any_synth_formant_kernel"
            return rep[name][0], pl.frames

        for n_fft in (int(n) for n in a.sizes.split(",")):
            q = nae.formant_lifter(48000, n_fft)
            kinds = [env for env in (False, True) if a.kernel in ("both", "env" if env else "formant")]
            for _ in range(a.warmup):
                for env in kinds:
                    timed(n_fft, q, env)
            runs = {env: [] for env in kinds}
            for _ in range(a.reps):
                for env in kinds:
                    runs[env].append(timed(n_fft, q, env))
            out = {"n_fft": n_fft, "lifter": q, "streams": n_streams, "frames_per_stream": S}
            for env in kinds:
                ms, frames = [r[0] for r in runs[env]], runs[env][0][1]
                med = float(np.median(ms))
                out["env" if env else "formant_pass3"] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "frames": frames,
                                                          "ns_per_frame": med * 1e6 / (frames * n_streams * ch)}
            if len(kinds) == 2:
                out["ratio"] = out["env"]["ns_per_frame"] / out["formant_pass3"]["ns_per_frame"]
            out["clock_ghz"] = ctx.clock_ghz()
            print(json.dumps(out), flush=True)
        d_x.free(); d_o.free()


if __name__ == "__main__":
    main()
