"""The CPU statement of the vocoder (tests/pv_ref/ref_pv.c) against the float64 synthesis tests/pv_f64.py fed the statement's own integer
phases: the pin behind Qs at EVERY tempo (the full float64 restatements hold at tempo 1/2 only), per stream-channel as
whole-signal RMS, worst hop block and worst sample.  The statement's distance is the floor the GPU tests multiply
(tests/test_gpu_pv_f64.py); here it is held under fixed caps, which are conditions on the inputs (broadband content wherever the envelope
stage runs), not measurements:
    without an envelope stage   e_rms <= 5e-7   e_blk <= 2e-6   e_max <= 3e-5
    with one                    e_rms <= 3e-6   e_blk <= 1e-5   e_max <= 3e-5
Then the instrument is shown to bite: four planted faults that the family's whole-signal 1e-4 lets through; and every synthesis and
transposer kernel name in csrc/ is some GPU case's expected kernel."""
import os
import re

import numpy as np
import pytest

import pv_f64
import pv_ref
import test_gpu_pv_f64
from conftest import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nodey-audio-editor_amd", "csrc")
PAIRS = [(1.5, 1 / 1.5), (0.7, 1 / 0.7), (0.25, 4.0), (1.0, 0.5), (1.0, 2 ** (-4 / 12)), (1.0, 2 ** (3 / 12)), (1.0, 2 ** (12 / 12))]
PHI = (0.5, 2 ** (4 / 12))
CAPS = {False: (5e-7, 2e-6, 3e-5), True: (3e-6, 1e-5, 3e-5)}
K = 16


def lifters(N):
    return (1, pv_ref.default_lifter(48000, N), N // 4)


# mode -> (channels, input kinds, options); "lifters": every lifter of lifters(N); "phis": every formant ratio, over SHIFT_PAIRS
MODES = {
    "plain": (1, pv_f64.KINDS, {}),
    "lock": (1, ("noise", "tones"), {"lock": True}),
    "transients": (1, ("clicks",), {"transients": True}),
    "link": (2, ("clicks",), {"transients": True, "link": True}),
    "formant": (1, ("noise", "tones"), {"lifters": True}),
    "formant+transients": (1, ("clicks",), {"transients": True, "lifters": True}),
    "formant-shift": (1, ("noise", "tones"), {"phis": True}),
}
# formant shift: A a pitch change and B a tempo change alone are PAIRS; C pitch 1 and rate != 1, D neither (the forced stage)
SHIFT_PAIRS = PAIRS + [(0.7, 1.0), (1.5, 1.0), (1.0, 1.0)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv_f64")))


def run(ref, x, ch, rate, pitch, N, lock=False, transients=False, link=False, lifter=0, phi=None, window=None):
    """(statement output, float64 synthesis, envelope stage on, onset verdicts or None)"""
    pl = pv_f64.get_plan(ref, rate, pitch, N, x.size // ch, lifter, phi)
    qs = on = None
    if pl.pv_on and not pv_f64.forced(pl):
        qs, on, _ = pv_ref.taps(ref, x, ch, rate, pitch, N, lock, transients, link)
    y = pv_ref.stretch(ref, x, ch, rate, pitch, N, lock, lifter, transients, phi, link)
    r = pv_f64.synth(ref, x, ch, rate, pitch, N, qs, lifter, phi, window)
    return y, r, pv_f64.envelope(pl, lifter, phi)[0] > 0, on


def variants(N, opts):
    base = {k: v for k, v in opts.items() if k in ("lock", "transients", "link")}
    if opts.get("lifters"):
        return [dict(base, lifter=q) for q in lifters(N)], PAIRS
    if opts.get("phis"):
        return [dict(base, lifter=pv_ref.default_lifter(48000, N), phi=phi) for phi in PHI], SHIFT_PAIRS
    return [base], PAIRS


@pytest.mark.parametrize("N,mode", [(N, m) for N in pv_ref.SIZES for m in MODES if m != "lock" or N == 1024])
def test_statement_is_pinned_at_every_tempo(ref, N, mode):
    ch, kinds, opts = MODES[mode]
    worst, n_env, shift_cases = {False: [0.0] * 3, True: [0.0] * 3}, 0, set()
    var, pairs = variants(N, opts)
    for v in var:
        for i, (rate, pitch) in enumerate(pairs):
            for j, kind in enumerate(kinds):
                x = pv_f64.content(kind, 6 * N + 777, ch, N, 7 + i + 3 * j)
                y, r, env, on = run(ref, x, ch, rate, pitch, N, **v)
                if v.get("transients"):
                    assert on.any(), (rate, pitch, "no onset")
                if "phi" in v:
                    shift_cases.add("D" if (rate, pitch) == (1.0, 1.0) else "C" if pitch == 1.0 else "B" if abs(rate * pitch - 1) < 1e-6 else "A")
                n_env += env
                for m in pv_f64.channel_measures(y, r, ch, N // 4):
                    worst[env] = [max(a, b) for a, b in zip(worst[env], m)]
                    assert all(a <= cap for a, cap in zip(m, CAPS[env])), (v, rate, pitch, kind, m, CAPS[env])
    print(f"N={N} {mode}: worst (e_rms, e_blk, e_max) plain {worst[False]}, with the envelope stage {worst[True]}")
    if opts.get("lifters") or opts.get("phis"):
        assert n_env > 0
    if opts.get("phis"):
        assert shift_cases == set("ABCD"), shift_cases


def test_the_lock_is_refused_elsewhere(ref):
    """why the pin has its lock rows at 1024 alone: at another size the lock is unsupported, in the statement as in the library"""
    x = pv_f64.content("noise", 4000, 1, 512, 1)
    for N in (512, 2048, 4096):
        assert pv_ref.stretch_rc(ref, x, 1, 1.5, 1 / 1.5, N, lock=True)[0] == -2


def test_transposer_alone(ref):
    """the float64 transposer (the table rounded to f32, the rest in double) against the statement's f32 taps, at the GPU cases' ratios"""
    x = pv_f64.content("tones", 6 * 1024 + 777, 2, 1024, 3)
    for rho in (0.26, 1509 / 768, 4.5, 12.0):
        y, r, env, _ = run(ref, x, 2, rho, 1.0, 1024)
        for m in pv_f64.channel_measures(y, r, 2, 256):
            print(f"rho {rho:.4g}: {m}")
            assert not env and all(a <= cap for a, cap in zip(m, CAPS[False])), (rho, m)


def test_measures_are_what_they_say():
    r = np.tile([2.0, -2.0], 300)                               # sigma = 2
    y = r.copy()
    y[130] += 0.5
    y[131] -= 0.5
    e_rms, e_blk, e_max = pv_f64.measures(y, r, 64)
    assert e_max == 0.25 and e_blk == np.sqrt(0.5 / 64) / 2 and abs(e_rms - np.sqrt(0.5 / 600) / 2) < 1e-15
    y = r.copy()
    y[599] += 1.0                                               # in the ragged last block of 24: it counts as a whole block
    assert pv_f64.measures(y, r, 64)[1] == np.sqrt(1.0 / 64) / 2
    with pytest.raises(AssertionError):
        pv_f64.measures(1e-4 * y, 1e-4 * r, 64)                 # sigma under 1e-3


FAULTS = ("one sample per hop off by 1e-3 sigma", "a gain of 1 + 5e-5", "one hop block times 1 + 1e-3", "one window entry off by 2^-12")


@pytest.mark.parametrize("rate,pitch", [(1.5, 1 / 1.5), (1.0, 2 ** (-4 / 12)), (1.0, 2 ** (3 / 12))])
@pytest.mark.parametrize("N", pv_ref.SIZES)
def test_planted_faults_are_caught(ref, N, rate, pitch):
    """each fault, planted into the statement's output, lifts at least one measure over K = 16 floors — the GPU tests' bar — while the
    first three stay under the whole-signal 1e-4 of the other tests: what that bar lets through.  The window fault is planted as the float64
    synthesis's own response to it (the statement's tables cannot be edited): entry N/2 + 3, where the window is near 1.  The input is
    48 N + 777 frames, the length of the other tests' signals: one block of b scaled by 1 + 1e-3 is 1e-3 / sqrt(b) of the whole, under 1e-4
    from 100 blocks on (here 128 and more)."""
    H = N // 4
    x = pv_f64.content("noise", 48 * N + 777, 1, N, 21)
    y, r, env, _ = run(ref, x, 1, rate, pitch, N)
    floor = pv_f64.measures(y, r, H)
    sigma = float(np.sqrt(np.mean(r * r)))
    y = y.astype(np.float64)
    w = pv_f64.hann32(N)
    w[N // 2 + 3] += 2.0 ** -12
    planted = [y.copy(), y * (1 + 5e-5), y.copy(), y + (run(ref, x, 1, rate, pitch, N, window=w)[1] - r)]
    planted[0][H // 3::H] += 1e-3 * sigma
    planted[2][5 * H:6 * H] *= 1 + 1e-3
    for name, z in zip(FAULTS, planted):
        m = pv_f64.measures(z, r, H)
        ratios = [a / b for a, b in zip(m, floor)]
        old = rel_rms(z, y)
        print(f"N={N} {rate:.3g}/{pitch:.3g} {name}: ratios to the floor {ratios}, rel RMS to the statement {old:.3g}")
        assert max(ratios) > K, (name, m, floor)
        if name != FAULTS[3]:
            assert old <= 1e-4, (name, old)


def test_formant_stage_needs_broadband_content(ref):
    """the conditioning of step 1: a purely harmonic input leaves most bins with rounding noise alone (1e-8 of the partials in f32, 1e-17 in
    double), log2 reads that noise, and the statement and the float64 synthesis part by orders of magnitude more than the caps; the same
    partials over noise 40 dB down meet them.  Not a fault of either: DESIGN.md §3, "Formant preservation" """
    N, rate, pitch = 1024, 1.0, 2 ** (4 / 12)
    n = 6 * N + 777
    t = np.arange(n)
    vowel = sum(0.3 / h * np.sin(2 * np.pi * 140.0 * h * t / 48000) for h in range(1, 30))
    floor = 0.003 * np.random.default_rng(5).standard_normal(n)
    q = pv_ref.default_lifter(48000, N)
    bare = pv_f64.measures(*run(ref, vowel.astype(np.float32), 1, rate, pitch, N, lifter=q)[:2], N // 4)
    over = pv_f64.measures(*run(ref, (vowel + floor).astype(np.float32), 1, rate, pitch, N, lifter=q)[:2], N // 4)
    print(f"harmonic series alone {bare}, over a noise floor {over}")
    assert bare[0] > 30 * CAPS[True][0], bare
    assert all(a <= cap for a, cap in zip(over, CAPS[True])), over


def launch_names():
    names = set()
    for f in ("kernels_pvpipe.hip", "kernels_pv_any.hip", "kernels_pvlock.hip", "kernels_pvenv.hip", "kernels_stft.hip", "kernels_resample.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            names |= set(re.findall(r'"([a-z0-9_]+_kernel)"', fh.read()))
    return names


def is_synthesis(name):
    return (name in ("pv_pipe_kernel", "pv_flow_kernel", "pv_env_kernel") or name.startswith("pv_any_synth") or name.startswith("pvlock_synth")
            or "resample" in name)


def test_every_synthesis_kernel_has_a_case():
    """the launch names in csrc/ that synthesise or transpose, against the kernels the GPU cases expect: a new instantiation fails here until a
    case measures it"""
    names = launch_names()
    synth = {n for n in names if is_synthesis(n)}
    want = ({"pv_pipe_kernel", "pv_flow_kernel", "pv_env_kernel", "resample_tile_kernel", "resample_kernel", "mix_resample_tile_kernel"}
            | {"pv_any_synth" + f + t + "_kernel" for f, t in (("", ""), ("_formant", ""), ("", "_transient"), ("_formant", "_transient"),
                                                               ("", "_link"), ("_formant", "_link"))}
            | {"pvlock_synth" + f + t + l + "_kernel" for f in ("", "_formant") for t in ("", "_transient") for l in ("", "_link")})
    assert want <= synth, want - synth                       # the reader finds the names it is meant to find
    covered = {c["kernel"] for c in test_gpu_pv_f64.CASES}
    assert synth <= covered, synth - covered
    assert covered <= names, covered - names                 # and no case expects a kernel that does not exist
    ids = [c["id"] for c in test_gpu_pv_f64.CASES]
    assert len(set(ids)) == len(ids)
