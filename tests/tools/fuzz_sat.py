#!/usr/bin/env python3
"""Randomised differential run (GPU box): the saturation K18, block entry and streaming handle, against its CPU statement
(tests/sat_ref/ref_sat.c), bit for bit.  A case draws the design's arguments over the whole range the header states, a length from the
kernel's edges (the halo, the pieces of 256, 512 and 1024 samples, the chunk) or a uniform one, the channel and stream counts, a view with
gaps or a shared source, the tiling (sat_tile) and, for one case in three, the handle with random put sizes from the host and the device in
turn.  draw() needs no device.
    python tests/tools/fuzz_sat.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import sat_ref
from block_gpu import CONFIGS, bits, mismatch, noise, statement
from fuzz_effects import pick
from sat_gpu import gpu_sat, sat_stream

SEEDED = (48, 3)                                                 # what tests/test_gpu_sat.py runs: cases, seed
EDGES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 319, 320, 511, 512, 513, 1023, 1024, 1025, 1087, 1088, 2047, 2048, 2049, 4 * 1024 + 3)


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)),
            design=(float(rng.uniform(0.0, 48.0)), float(pick(rng, (0.0, 0.0, float(rng.uniform(0.0, 1.0))))), int(rng.integers(2)),
                    int(pick(rng, sat_ref.FACTORS)), float(rng.uniform(-24.0, 24.0)), float(pick(rng, (1.0, float(rng.uniform(0.0, 1.0)))))),
            n=int(pick(rng, EDGES)) if rng.integers(2) else int(rng.integers(1, 20000)),
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 9, 130))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0,
            level_db=float(rng.uniform(-40.0, 6.0)), tile=int(pick(rng, (0, 0, 1, 2, 3, 5))),
            handle=handle, puts=tuple(int(k) for k in rng.integers(1, 3000, 8)))


def run_case(nae, ctx, L, case):
    p = sat_ref.design(*case["design"])
    rng = np.random.default_rng(case["seed"])
    x = noise(rng, case["n_streams"], case["n"], case["ch"], case["shared"]) * np.float32(10.0 ** (case["level_db"] / 20.0))
    ctx.debug_set("sat_tile", case["tile"])
    try:
        if case["handle"]:
            got, want = sat_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], sat_ref.run_tail(L, p, x[0])[None]
        else:
            got = gpu_sat(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"])
            want = np.repeat(sat_ref.run(L, p, x[0])[None], len(x), axis=0) if case["shared"] else sat_ref.run_streams(L, p, x)
    finally:
        ctx.debug_set("sat_tile", 0)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(sat_ref)
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
    print(f"fuzz_sat: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
