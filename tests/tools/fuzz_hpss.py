#!/usr/bin/env python3
"""Randomised differential run (GPU box): the separation K21, block entry and streaming handle, against its CPU statement
(tests/hpss_ref/ref_hpss.c), bit for bit.  A case draws the frame size, the two spans over 0 ... 8 (their edges more often), the mask, two
levels over the whole range the header states (-120 dB, gain 0, more often), a length from the hop's edges or a uniform one, a forced tile or
the library's, a signal of wandering noise with clicks and a tone in it, the channel and stream counts, a view with gaps or a shared source
and, for one case in three, the handle with random put sizes from the host and the device in turn.  draw() needs no device;
tests/test_hpss_cpu.py pins, without a GPU, which edges SEEDED reaches.
    python tests/tools/fuzz_hpss.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import hpss_ref
from block_gpu import CONFIGS, mismatch, statement
from fuzz_effects import pick
from hpss_gpu import gpu_hpss, hpss_stream

SEEDED = (24, 7)                                                 # what tests/test_gpu_hpss.py runs: cases, seed


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        n_fft = int(pick(rng, hpss_ref.SIZES))
        H = n_fft // 4
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)), n_fft=n_fft,
            time_span=int(pick(rng, (0, 1, 8, int(rng.integers(0, 9))))), freq_span=int(pick(rng, (0, 1, 8, int(rng.integers(0, 9))))),
            mask=hpss_ref.MASKS[int(rng.integers(2))],
            harmonic_db=float(pick(rng, (-120.0, 0.0, float(rng.uniform(-120.0, 12.0))))), percussive_db=float(pick(rng, (-120.0, 0.0, float(rng.uniform(-120.0, 12.0))))),
            n=int(pick(rng, (1, H - 1, H, H + 1, n_fft, n_fft + 1, 5 * H + 7))) if rng.integers(2) else int(rng.integers(1, 24 * H)),
            tile=int(pick(rng, (0, 0, 1, 2, 3, 7))),
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 9))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0,
            click_every=int(rng.integers(50, 3000)), tone=float(rng.uniform(0.001, 0.3)),
            handle=handle, puts=tuple(int(k) for k in rng.integers(1, 3 * H, 8)))


def signal(case):
    """[streams, n, ch] f32: K13's wandering noise under a tone and a click train, another phase per stream"""
    rng = np.random.default_rng(case["seed"])
    n_streams, n, ch = case["n_streams"], case["n"], case["ch"]
    x = hpss_ref.wander(rng, n_streams, n, ch, level=0.05, period=3.0 * case["n_fft"]).astype(np.float64)
    t = np.arange(n)[None, :, None] + rng.integers(0, case["click_every"], (n_streams, 1, 1))
    x += 0.3 * np.sin(case["tone"] * t) + 0.9 * (t % case["click_every"] == 0)
    x = x.astype(np.float32)
    if case["shared"]:
        x[:] = x[0]
    return x


def params(nae, case):
    p = nae.Context.hpss_design(case["harmonic_db"], case["percussive_db"], case["n_fft"], case["time_span"], case["freq_span"], case["mask"])
    return hpss_ref.Params(p.n_fft, p.time_span, p.freq_span, p.hard, p.gain_h, p.gain_p)


def run_case(nae, ctx, L, case):
    p, x = params(nae, case), signal(case)
    ctx.debug_set("hpss_tile", case["tile"])
    try:
        if case["handle"]:
            got, want = hpss_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], hpss_ref.run(L, p, x[0])[None]
        else:
            got = gpu_hpss(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"])
            want = np.repeat(hpss_ref.run(L, p, x[0])[None], len(x), axis=0) if case["shared"] else hpss_ref.run_streams(L, p, x)
    finally:
        ctx.debug_set("hpss_tile", 0)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(hpss_ref)
    done = 0
    try:
        for case in draw(cases, seed):
            message = run_case(nae, ctx, L, case)
            assert not message, (case, message)
            done += 1
    finally:
        if own:
            ctx.close()
    return done


if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    n_seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    print(f"fuzz_hpss: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
