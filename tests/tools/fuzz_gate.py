#!/usr/bin/env python3
"""Randomised differential run (GPU box): the gate K19, block entry and streaming handle, against its CPU statement
(tests/gate_ref/ref_gate.c), bit for bit.  A case draws the design's arguments over the whole range the header states (the hold and the
look-ahead also from the lane's, the chunk's and the limits' edges), a length from the kernel's edges or a uniform one, a signal of bursts
and gaps around the thresholds, the channel and stream counts, a view with gaps or a shared source and, for one case in three, the handle
with random put sizes from the host and the device in turn.  draw() needs no device.
    python tests/tools/fuzz_gate.py [cases=60] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import gate_ref
from block_gpu import CONFIGS, mismatch, statement
from fuzz_effects import pick
from gate_gpu import gate_stream, gpu_gate

SEEDED = (36, 5)                                                 # what tests/test_gpu_gate.py runs: cases, seed
EDGES = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 7)
RATE = 48000


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        la = int(pick(rng, (0, 0, 1, 15, 16, 17, 1023, 1024, int(rng.integers(0, 1025)))))
        hold = int(pick(rng, (0, 1, 15, 16, 17, 1024, 5000, int(rng.integers(0, 3000)))))
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)),
            design=(RATE, gate_ref.MODES[int(rng.integers(2))], float(rng.uniform(-90.0, 0.0)), float(pick(rng, (0.0, float(rng.uniform(0.0, 24.0))))),
                    float(rng.uniform(0.0, 120.0)), float(rng.uniform(1.0, 100.0)), float(pick(rng, (0.0, float(rng.uniform(0.0, 0.5))))),
                    hold / RATE, float(rng.uniform(0.001, 5.0)), la / RATE, int(rng.integers(2))),
            hold=hold, lookahead=la,
            n=int(pick(rng, EDGES)) if rng.integers(2) else int(rng.integers(1, 12000)),
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 9, 130))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0,
            period=int(rng.integers(20, 4000)), duty=float(rng.uniform(0.02, 0.6)), spread_db=float(rng.uniform(0.0, 30.0)),
            handle=handle, puts=tuple(int(k) for k in rng.integers(1, 3000, 8)))


def signal(case):
    """[streams, n, ch] f32: noise in bursts above the opening threshold over a floor around the closing one, another phase per stream"""
    rng = np.random.default_rng(case["seed"])
    n_streams, n, ch = case["n_streams"], case["n"], case["ch"]
    thr = case["design"][2]
    t = np.arange(n)[None, :, None] + rng.integers(0, case["period"], (n_streams, 1, 1))
    on = (t % case["period"]) < case["duty"] * case["period"]
    level_db = np.where(on, thr + 6.0, thr - case["design"][3] - 3.0) + rng.uniform(-case["spread_db"], case["spread_db"], (n_streams, n, ch)) / 2.0
    x = (rng.choice([-1.0, 1.0], (n_streams, n, ch)) * 10.0 ** (level_db / 20.0)).astype(np.float32)
    if case["shared"]:
        x[:] = x[0]
    return x


def params(case):
    p = gate_ref.design(*case["design"])
    assert (p.hold, p.lookahead) == (case["hold"], case["lookahead"]), "the design's rounding gives the drawn sample counts"
    return p


def run_case(nae, ctx, L, case):
    p, x = params(case), signal(case)
    if case["handle"]:
        got, want = gate_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], gate_ref.run(L, p, x[0])[None]
    else:
        got = gpu_gate(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"])
        want = np.repeat(gate_ref.run(L, p, x[0])[None], len(x), axis=0) if case["shared"] else gate_ref.run_streams(L, p, x)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(gate_ref)
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
    print(f"fuzz_gate: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
