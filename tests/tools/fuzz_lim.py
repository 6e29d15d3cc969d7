#!/usr/bin/env python3
"""Randomised differential run (GPU box): the limiter K22, block entry and streaming handle, against its CPU statement
(tests/lim_ref/ref_lim.c), bit for bit.  A case draws the design's arguments over the whole range the header states (the look-ahead also
from the lane's and the limit's edges, the ceiling, the drive and the release from theirs), a length from the kernel's edges or a uniform
one, a signal of noise in bursts with full-scale peaks at drawn positions (also around the chunk borders and the signal's end), the channel
and stream counts, a view with gaps or a shared source and, for one case in three, the handle with random put sizes from the host and the
device in turn.  draw() needs no device.
    python tests/tools/fuzz_lim.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import lim_ref
from block_gpu import CONFIGS, mismatch, statement
from fuzz_effects import pick
from lim_gpu import gpu_lim, lim_stream

SEEDED = (36, 5)                                                 # what tests/test_gpu_lim.py runs: cases, seed
EDGES = (1, 5, 6, 7, 15, 16, 17, 1018, 1023, 1024, 1025, 1030, 2047, 2048, 2049, 3 * 1024 + 7)
RATE = 48000


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        la = int(pick(rng, (0, 0, 1, 15, 16, 17, 72, 1017, 1018, int(rng.integers(0, 1019)))))
        n = int(pick(rng, EDGES)) if rng.integers(2) else int(rng.integers(1, 12000))
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)),
            design=(RATE, float(pick(rng, (-20.0, 0.0, -1.0, float(rng.uniform(-20.0, 0.0))))), float(pick(rng, (-24.0, 24.0, 0.0, float(rng.uniform(-24.0, 24.0))))),
                    float(pick(rng, (0.001, 5.0, float(rng.uniform(0.001, 5.0))))), la / RATE, int(rng.integers(2)), int(rng.integers(2))),
            lookahead=la, n=n,
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 9, 130))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0,
            period=int(rng.integers(20, 4000)), duty=float(rng.uniform(0.02, 0.9)), floor_db=float(rng.uniform(-60.0, -6.0)),
            peaks=tuple(int(pick(rng, (0, n - 1, 1017, 1018, 1023, 1024, 1029, 1035, 2047, int(rng.integers(0, n))))) for _ in range(int(rng.integers(0, 6)))),
            handle=handle, puts=tuple(int(k) for k in rng.integers(1, 3000, 8)))


def signal(case):
    """[streams, n, ch] f32: noise in bursts over a floor, another phase per stream, and full-scale samples at the drawn positions"""
    rng = np.random.default_rng(case["seed"])
    n_streams, n, ch = case["n_streams"], case["n"], case["ch"]
    t = np.arange(n)[None, :, None] + rng.integers(0, case["period"], (n_streams, 1, 1))
    on = (t % case["period"]) < case["duty"] * case["period"]
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * np.where(on, 1.0, 10.0 ** (case["floor_db"] / 20.0))).astype(np.float32)
    for k, at in enumerate(case["peaks"]):
        if 0 <= at < n:
            x[k % n_streams, at, k % ch] = 1.0 if k % 2 else -1.0
    if case["shared"]:
        x[:] = x[0]
    return x


def params(case):
    p = lim_ref.design(*case["design"])
    assert p.lookahead == case["lookahead"], "the design's rounding gives the drawn sample count"
    return p


def run_case(nae, ctx, L, case):
    p, x = params(case), signal(case)
    if case["handle"]:
        got, want = lim_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], lim_ref.run(L, p, x[0])[None]
    else:
        got = gpu_lim(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"])
        want = np.repeat(lim_ref.run(L, p, x[0])[None], len(x), axis=0) if case["shared"] else lim_ref.run_streams(L, p, x)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(lim_ref)
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
    print(f"fuzz_lim: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
