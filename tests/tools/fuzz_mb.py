#!/usr/bin/env python3
"""Randomised differential run (GPU box): the multiband compressor K20, block entry and streaming handle, against its CPU statement
(tests/mb_ref/ref_mb.c), bit for bit.  A case draws the band count, ascending crossovers between 20 Hz and 0.45 of the rate, every band's
design arguments over the range the header states, one look-ahead and link for all bands (the look-ahead also from the lane's and the chunk's
edges), the mute and bypass masks, a length from the kernel's edges or a uniform one, a signal whose level wanders around the thresholds, the
channel and stream counts, a view with gaps or a shared source, the slab and the group (debug keys mb_slab, mb_group) and, for one case in
three, the handle with random put sizes from the host and the device in turn.  draw() needs no device.
    python tests/tools/fuzz_mb.py [cases=60] [seed=1]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np
import dyn_ref
import mb_ref
from block_gpu import CONFIGS, mismatch, statement
from fuzz_effects import pick
from mb_gpu import debug_keys, gpu_mb, mb_stream

SEEDED = (20, 7)                                                 # what tests/test_gpu_mb.py runs: cases, seed
EDGES = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 7, 5 * 1024 + 7)
RATES = (8000, 44100, 48000, 96000)


def draw(cases, seed):
    """the case records: plain dicts"""
    rng = np.random.default_rng(seed)
    for i in range(cases):
        ch, _, sl, dl, shared = CONFIGS[int(rng.integers(len(CONFIGS)))]
        handle = i % 3 == 2
        rate = int(pick(rng, RATES))
        n_bands = int(rng.integers(2, 5))
        la = int(pick(rng, (0, 0, 1, 15, 16, 17, 1023, 1024, int(rng.integers(0, 1025)))))
        link = int(rng.integers(2))
        xs = np.sort(np.exp(rng.uniform(np.log(20.0), np.log(0.45 * rate), n_bands - 1)))
        for k in range(1, len(xs)):                                  # strictly ascending, and apart
            xs[k] = max(xs[k], xs[k - 1] * 1.05)
        bands = [(rate, float(rng.uniform(-60.0, 0.0)), float(pick(rng, (1.0, float("inf"), float(rng.uniform(1.0, 20.0))))), float(pick(rng, (0.0, float(rng.uniform(0.0, 24.0))))),
                  float(pick(rng, (0.0, float(rng.uniform(0.0, 0.5))))), float(rng.uniform(0.001, 5.0)), la / rate, float(rng.uniform(-24.0, 24.0)), link)
                 for _ in range(n_bands)]
        yield dict(
            index=i, seed=int(rng.integers(1 << 31)), rate=rate, n_bands=n_bands, crossovers=tuple(float(f) for f in xs), bands=bands, lookahead=la,
            mute=int(rng.integers(1 << n_bands)) if rng.integers(3) == 0 else 0, bypass=int(rng.integers(1 << n_bands)) if rng.integers(3) == 0 else 0,
            n=int(pick(rng, EDGES)) if rng.integers(2) else int(rng.integers(1, 9000)),
            ch=ch, n_streams=1 if handle else int(pick(rng, (1, 2, 3, 9, 70))), src=sl, dst=dl, shared=shared and not handle,
            gap=int(rng.integers(0, 9)) if sl == "p" else 0, chan_pad=int(rng.integers(0, 9)) if "p" in (sl, dl) else 0,
            period=int(rng.integers(50, 4000)), level_db=float(rng.uniform(-40.0, -3.0)),
            slab=int(pick(rng, (0, 0, 1, 2, 3))), group=int(pick(rng, (0, 0, 1, 2, 5))),
            handle=handle, puts=tuple(int(k) for k in rng.integers(1, 3000, 8)))


def signal(case):
    """[streams, n, ch] f32: noise whose level wanders +-14 dB around level_db, another phase per stream and channel"""
    rng = np.random.default_rng(case["seed"])
    n_streams, n, ch = case["n_streams"], case["n"], case["ch"]
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * 10.0 ** ((case["level_db"] + 14.0 * np.sin(2 * np.pi * t / case["period"] + ph)) / 20.0)).astype(np.float32)
    if case["shared"]:
        x[:] = x[0]
    return x


def params(L, case):
    bands = []
    for args in case["bands"]:
        b = dyn_ref.Params()
        assert L.ref_dyn_design(*args, C.byref(b)) == 0, args
        assert b.lookahead == case["lookahead"], "the design's rounding gives the drawn look-ahead"
        bands.append(b)
    p = mb_ref.design(L, case["rate"], case["crossovers"], bands, case["mute"], case["bypass"])
    assert p is not None, case
    return p


def run_case(nae, ctx, L, case):
    p, x = params(L, case), signal(case)
    with debug_keys(ctx, mb_slab=case["slab"], mb_group=case["group"]):
        if case["handle"]:
            got, want = mb_stream(nae, ctx, p, x[0], case["puts"], device=(False, True))[None], mb_ref.run(L, p, x[0])[None]
        else:
            got = gpu_mb(nae, ctx, p, x, case["src"], case["dst"], case["shared"], gap=case["gap"], chan_pad=case["chan_pad"])
            want = np.repeat(mb_ref.run(L, p, x[0])[None], len(x), axis=0) if case["shared"] else mb_ref.run_streams(L, p, x)
    return mismatch(got, want)


def main(cases=60, seed=1, ctx=None, nae=None):
    """runs the cases; returns how many matched (an assertion names the first that did not)"""
    own = ctx is None
    if own:
        import naeload
        nae = naeload.load()
        ctx = nae.Context(0)
    L = statement(mb_ref)
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
    print(f"fuzz_mb: {main(n_cases, n_seed)} of {n_cases} cases match the statement bit for bit (seed {n_seed})")
