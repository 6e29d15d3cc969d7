#!/usr/bin/env python3
"""Randomised differential run (GPU box): the dither K23, block entry and streaming handle, against its CPU statement
(tests/dither_ref/ref_dither.c), bit for bit.  A case draws the word length, the dither's kind, a preset or 1 ... 12 drawn taps (also at an
absolute sum just under 64), a seed (also 0 and 2^64 - 1), a length from the kernels' edges or a uniform one, a signal of noise at a drawn level
(also far over full scale, and with samples that are not finite), the channel and stream counts (also more than one wave and a partly filled
one), a view with gaps or a shared source, who does the feed-forward work (debug key dither_roles) and, for one case in three, the handle
with random put sizes from the host and the device in turn.  draw() needs no device.
    python tests/tools/fuzz_dither.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import dither_ref
from block_gpu import CONFIGS, mismatch, statement
from dither_gpu import dither_stream, gpu_dither
from fuzz_effects import pick

SEEDED = (36, 5)                                                 # what tests/test_gpu_dither.py runs: cases, seed
EDGES = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4099)


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        k = int(pick(rng, (0, 0, 1, 2, 5, 12, int(rng.integers(1, 13)))))
        total = float(pick(rng, (63.99, 1.0, float(rng.uniform(0.1, 8.0)))))   # just inside the limit: the scaled taps' sum is rounded
        preset = pick(rng, ("first", "second", "lipshitz", None, None))
        taps = dither_ref.PRESETS[preset] if (preset and k) else dither_ref.drawn_taps(int(rng.integers(1 << 31)), k, total) if k else ()
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)), bits=int(pick(rng, (8, 16, 24, int(rng.integers(8, 25))))), kind=int(rng.integers(4)), taps=taps,
            dither_seed=int(pick(rng, (0, 1, 2 ** 64 - 1, int(rng.integers(1 << 62))))),
            n=int(pick(rng, EDGES)) if rng.integers(2) else int(rng.integers(1, 9000)),
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 31, 33, 65, 130))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0, offset=int(rng.integers(2)),
            level=float(pick(rng, (1.0, 1.3, 1e-4, 1e30, float(10.0 ** rng.uniform(-5, 0.5))))), bad=int(rng.integers(0, 4)),
            roles=int(pick(rng, (0, 1, 2))), handle=handle, puts=tuple(int(v) for v in rng.integers(1, 3000, 8)))


def signal(case):
    """[streams, n, ch] f32: noise at the drawn level, and `bad` samples that are not finite at drawn places"""
    rng = np.random.default_rng(case["seed"])
    n_streams, n, ch = case["n_streams"], case["n"], case["ch"]
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * case["level"]).astype(np.float32)
    for k in range(case["bad"]):
        x[int(rng.integers(n_streams)), int(rng.integers(n)), int(rng.integers(ch))] = (np.nan, np.inf, -np.inf)[k % 3]
    if case["shared"]:
        x[:] = x[0]
    return x


def params(case):
    return dither_ref.params(case["bits"], case["kind"], case["taps"], case["dither_seed"])


def run_case(nae, ctx, L, case):
    p, x = params(case), signal(case)
    ctx.debug_set("dither_roles", case["roles"])
    try:
        if case["handle"]:
            got, want = dither_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], dither_ref.run(L, p, x[0])[None]
        else:
            got = gpu_dither(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"], offset=case["offset"])
            want = dither_ref.run_streams(L, p, x, case["shared"])
    finally:
        ctx.debug_set("dither_roles", 0)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(dither_ref)
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
    print(f"fuzz_dither: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
