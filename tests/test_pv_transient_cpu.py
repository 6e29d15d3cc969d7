"""Transient preservation of the K7 vocoder ("Transient preservation"), no GPU: the CPU statement
(tests/pv_ref/ref_pv.c) without the flag is the oracle and the recorded phases, its onset rule is a numpy float32 restatement of
the specification's, attacks stay sharp, steady signals give no onset, and the C ABI, the binding and the host nodes carry the flag."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_ref
from pv_gpu import RANGE_RHOS, RANGE_TEMPOS, hard_bursts, placed_clicks, range_case, tone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (512, 1024, 2048, 4096)
RISE, FLOOR, NUM, DEN = np.float32(4.0), np.float32(2.0 ** -20), 3, 8     # include/nae_dsp_spec.h
SR = 48000
# the four node settings of "no false onsets": velocity 0.6 / 1.5 with keep_pitch, pitch +3 / -7 semitones (both stage orders)
SETTINGS = [(0.6, 1 / 0.6), (1.5, 1 / 1.5), (1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12))]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def phase_digest(qs):
    return hashlib.sha256(np.ascontiguousarray(qs, "<i4").tobytes()).hexdigest()


def faded(x, m=960):
    """a 20 ms raised-cosine fade-out: an abrupt end is itself an attack (its splatter rises in every bin far from the signal's own).  The
    start needs none: its first frames are high from frame 1 on, and frame 1 never fires."""
    x = np.asarray(x, np.float64).copy()
    x[-m:] *= 0.5 + 0.5 * np.cos(np.pi * np.arange(m) / m)
    return x.astype(np.float32)


@pytest.mark.parametrize("n_fft", SIZES)
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5)])
def test_unflagged_statement_is_the_vocoder_statement(ref, n_fft, ch, rate, pitch):
    """transients = 0 — every size, the lock at 1024, mono and stereo, both stage orders (pitch up: transposer first): at 1024 unlocked with
    lifter 0 the samples are the oracle's bit for bit; in every case the integer synthesis phases of every frame are those recorded in
    tests/golden/pv_option_phase.json ("unflagged ...": sha256 of the int32 [frames][ch][N/2 + 1] array) from the
    statement this one replaced, at commit 602aacf, where the unflagged transient statement was tested equal to it.  And the flag changes
    nothing on a steady input: with the 20 ms fade-out of test_no_false_onsets, transients = 1 gives the bits of transients = 0, samples
    (lifter 0 and the default lifter) and phases.  (Without the fade the two-tone's abrupt end fires one onset, in a frame whose window spans
    the end, in every case here — at 602aacf too — so the fade is part of the claim.)"""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pv_option_phase.json")))
    L = 12000
    m = tone(L)
    x = np.stack([m, 0.5 * m], 1).reshape(-1) if ch == 2 else m
    xf = np.stack([faded(m), faded(0.5 * m)], 1).reshape(-1) if ch == 2 else faded(m)
    locks = (False, True) if n_fft == 1024 else (False,)
    for lock in locks:
        if n_fft == 1024 and not lock:
            assert same_bits(pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, transients=False), orc.stretch(x, ch, rate, pitch))
        key = f"unflagged {rate!r} {pitch!r} ch{ch} {n_fft}" + (" locked" if lock else "")
        assert phase_digest(pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock, transients=False)) == golden[key], key
        for q in (0, pv_ref.default_lifter(SR, n_fft)):
            a = pv_ref.stretch(ref, xf, ch, rate, pitch, n_fft, lock, q, transients=True)
            b = pv_ref.stretch(ref, xf, ch, rate, pitch, n_fft, lock, q, transients=False)
            assert same_bits(a, b), (lock, q)
        assert np.array_equal(pv_ref.synth_phase(ref, xf, ch, rate, pitch, n_fft, lock, transients=True),
                              pv_ref.synth_phase(ref, xf, ch, rate, pitch, n_fft, lock, transients=False)), lock


def numpy_onsets(P, n_fft):
    """§1's rule in numpy float32: rise iff P_f > RISE P_{f-1} and P_f > FLOOR N (a NaN compares false); high iff DEN c >= NUM B; onset iff
    f >= 2, high(f) and not high(f - 1)"""
    P = np.asarray(P, np.float32)
    frames, B = P.shape
    on = np.zeros(frames, bool)
    high_prev = False
    for f in range(1, frames):
        with np.errstate(invalid="ignore", over="ignore"):
            rise = (P[f] > RISE * P[f - 1]) & (P[f] > FLOOR * np.float32(n_fft))
        high = DEN * int(rise.sum()) >= NUM * B
        on[f] = f >= 2 and high and not high_prev
        high_prev = high
    return on


@pytest.mark.parametrize("n_fft", SIZES)
def test_onset_rule_on_synthetic_spectra(ref, n_fft):
    """ties, NaN, Inf, the floor, exact quadrupling and a count exactly at (and one below) the threshold: the statement's rule equals the
    numpy restatement, and the hand-made cases give the verdicts the specification says"""
    B = n_fft // 2 + 1
    need = -(-NUM * B // DEN)                       # the least count that is high
    fl = np.float32(FLOOR * np.float32(n_fft))
    base = np.full(B, 1.0, np.float32)

    def frame_with(k, value, rest=1.0):
        p = np.full(B, rest, np.float32)
        p[:k] = value
        return p

    cases = {
        "at threshold": ([base, base, frame_with(need, 8.0)], [False, False, True]),
        "one below": ([base, base, frame_with(need - 1, 8.0)], [False, False, False]),
        "exact x4 does not rise": ([base, base, np.full(B, 4.0, np.float32)], [False, False, False]),
        "just above x4": ([base, base, np.full(B, np.nextafter(np.float32(4.0), np.float32(5.0)), np.float32)], [False, False, True]),
        "tie with previous": ([base, base, base], [False, False, False]),
        "at the floor": ([np.zeros(B, np.float32)] * 2 + [np.full(B, fl, np.float32)], [False, False, False]),
        "above the floor": ([np.zeros(B, np.float32)] * 2 + [np.full(B, np.nextafter(fl, np.float32(1)), np.float32)], [False, False, True]),
        "NaN now": ([base, base, np.full(B, np.nan, np.float32)], [False, False, False]),
        "NaN before": ([base, np.full(B, np.nan, np.float32), np.full(B, 8.0, np.float32)], [False, False, False]),
        "Inf now": ([base, base, np.full(B, np.inf, np.float32)], [False, False, True]),
        "Inf before": ([base, np.full(B, np.inf, np.float32), np.full(B, np.inf, np.float32)], [False, False, False]),
        "frame 1 never fires": ([np.zeros(B, np.float32), np.ones(B, np.float32)], [False, False]),
        "high twice fires once": ([base, base, np.full(B, 8.0, np.float32), np.full(B, 64.0, np.float32), np.full(B, 64.0, np.float32),
                                   np.full(B, 512.0, np.float32)], [False, False, True, False, False, True]),
    }
    for name, (frames, want) in cases.items():
        P = np.stack(frames)
        got = pv_ref.onset_rule(ref, P, n_fft)
        assert list(got) == want, name
        assert np.array_equal(got, numpy_onsets(P, n_fft)), name
    rng = np.random.default_rng(n_fft)
    for trial in range(20):
        P = (rng.exponential(1.0, (12, B)) * rng.choice([1e-9, 1.0, 8.0, 100.0], (12, 1))).astype(np.float32)
        P[rng.random(P.shape) < 0.01] = np.nan
        assert np.array_equal(pv_ref.onset_rule(ref, P, n_fft), numpy_onsets(P, n_fft)), trial


def click_train():
    L = 96000
    x = np.zeros(L, np.float32)
    pos = np.arange(4800, L - 4800, 9600)
    x[pos] = 1.0
    return x, pos


def click_width(ref, n_fft, transients):
    """the width of tests/test_pv_sizes_cpu.py's click_width on the flagged or unflagged statement"""
    x, pos = click_train()
    y = pv_ref.stretch(ref, x, 1, 1.5, 1 / 1.5, n_fft, transients=transients).astype(np.float64)
    widths = []
    for p in pos:
        c = int(round(p / 1.5))
        e = y[c - 3000:c + 3000] ** 2
        t = np.arange(e.size)
        m = (e * t).sum() / e.sum()
        widths.append(np.sqrt((e * (t - m) ** 2).sum() / e.sum()))
    return float(np.median(widths))


def test_attacks_stay_sharp(ref):
    """the click train at velocity 1.5: exactly one onset per click (on a frame whose window holds it), and the flagged width is at most half
    the unflagged one at 1024 / 2048 / 4096, and at 4096 no wider than the unflagged 1024.  Measured RMS widths, unflagged / flagged:
    75 / 0.00001, 208 / 0.00002, 327 / 3.3, 709 / 0.0001 samples at 512 / 1024 / 2048 / 4096 (a single-sample click comes back a single sample)"""
    x, pos = click_train()
    for n_fft in SIZES:
        on = pv_ref.onsets(ref, x, 1, 1.5, 1 / 1.5, n_fft)[:, 0]
        f = np.nonzero(on)[0]
        assert f.size == pos.size, (n_fft, f)
        _, pl = pv_ref.plan(ref, 1.5, 1 / 1.5, n_fft, x.size)
        starts = ((f - 1) * pl.ha_q24 + (1 << 23) >> 24) - n_fft // 2
        for p, s in zip(pos, starts):
            assert s <= p < s + n_fft, (n_fft, p, s)
    w = {n: (click_width(ref, n, False), click_width(ref, n, True)) for n in SIZES}
    for n in (1024, 2048, 4096):
        assert w[n][1] <= 0.5 * w[n][0], w
    assert w[4096][1] <= w[1024][0], w


def steady_signals():
    n = 96000
    t = np.arange(n) / SR
    k = np.log(15000.0 / 50.0)
    f_vib = 440.0 + 20.0 * np.sin(2 * np.pi * 5.0 * t)
    return {
        "two-tone": 0.3 * np.sin(2 * np.pi * 110 * t) + 0.3 * np.sin(2 * np.pi * 140 * t),
        "sweep": 0.5 * np.sin(2 * np.pi * 50.0 * (n / SR) / k * (np.exp(t / (n / SR) * k) - 1)),
        "vibrato": 0.5 * np.sin(2 * np.pi * np.cumsum(f_vib) / SR),
        "noise": 0.1 * np.random.default_rng(5).standard_normal(n),
    }


def bursts():
    """a sustained C major chord with 8 decaying noise bursts, 4 s"""
    n = 192000
    t = np.arange(n) / SR
    x = sum(0.15 * np.sin(2 * np.pi * f * t) for f in (261.63, 329.63, 392.0))
    rng = np.random.default_rng(7)
    pos = [int((i + 0.5) * n / 8) for i in range(8)]
    for p in pos:
        x[p:p + 4800] += 0.5 * np.exp(-np.arange(4800) / 600.0) * rng.standard_normal(4800)
    return faded(x), pos


@pytest.mark.parametrize("n_fft", SIZES)
def test_no_false_onsets(ref, n_fft):
    """the 110 + 140 Hz two-tone, a 50 Hz - 15 kHz log sweep over 2 s, a 5 Hz vibrato and steady white noise (sigma 0.1), each with a 20 ms
    fade-out, at the four node settings: no onset, and the flagged output is the unflagged one bit for bit.  The chord with 8 noise bursts: one
    onset per burst, on a frame whose window holds the burst's start."""
    for name, x in steady_signals().items():
        x = faded(x)
        for rate, pitch in SETTINGS:
            assert not pv_ref.onsets(ref, x, 1, rate, pitch, n_fft).any(), (name, rate, pitch)
            assert same_bits(pv_ref.stretch(ref, x, 1, rate, pitch, n_fft, transients=True),
                             pv_ref.stretch(ref, x, 1, rate, pitch, n_fft, transients=False)), (name, rate, pitch)
    x, pos = bursts()
    for rate, pitch in SETTINGS:
        on = pv_ref.onsets(ref, x, 1, rate, pitch, n_fft)[:, 0]
        f = np.nonzero(on)[0]
        assert f.size == len(pos), (rate, pitch, f)
        _, pl = pv_ref.plan(ref, rate, pitch, n_fft, x.size)
        starts = ((f - 1) * pl.ha_q24 + (1 << 23) >> 24) - n_fft // 2
        scale = pl.rate_eff if pl.rs_first else 1.0          # transposer first: the vocoder reads the transposed signal
        for p, s in zip(pos, starts):
            assert s <= p / scale < s + n_fft, (rate, pitch, p, s)


@pytest.mark.parametrize("n_fft", SIZES)
def test_range_rows_fire_in_one_channel_only(nae, ref, n_fft):
    """the premise of tests/test_gpu_pv_transient.py::test_transients_over_the_tempo_range, where it can be checked: in every row (tempo
    0.26, 3.9, 8, 16 and 1/64, the transposer off, behind and in front) the statement has an onset in the left channel only and one in the
    right only; above tempo 1/2 the placed clicks' onsets fall on a 16-frame tile's first, second and last frame.  At 1/64 the analysis hop
    is N/256 samples and nothing within full scale fires — the same clicks at height 0.9, and the hard bursts that fire at 0.26, give no
    onset — while the clicks of height 4096 in digital silence that the rows use do."""
    for tempo in RANGE_TEMPOS:
        for rho in RANGE_RHOS:
            x, L, rate, pitch = range_case(nae, n_fft, tempo, rho)
            on = pv_ref.onsets(ref, x, 2, rate, pitch, n_fft)
            assert 48 <= on.shape[0] <= 1200, (tempo, rho, on.shape)
            left, right = np.nonzero(on[:, 0] & ~on[:, 1])[0], np.nonzero(on[:, 1] & ~on[:, 0])[0]
            assert left.size and right.size, (tempo, rho, left, right)
            if tempo > 0.5:
                assert {0, 1, 15} <= set(np.nonzero(on.any(1))[0] % 16), (tempo, rho)
            if tempo < 1 / 32:
                H, Lb = n_fft // 4, int(14 * n_fft * max(rho, 1.0))              # two bursts
                for quiet in (placed_clicks(nae, L, 2, rate, pitch, n_fft, first=1, every=1, depth=int(H * tempo), sides=True),
                              hard_bursts(nae, Lb, rate, pitch, n_fft)):
                    assert np.abs(quiet).max() > 0.5 and not pv_ref.onsets(ref, quiet, 2, rate, pitch, n_fft).any(), (tempo, rho)


def test_abi_declares_the_flag(nae):
    h = open(os.path.join(ROOT, "include", "nae_gpu.h")).read()
    assert re.search(r"#define\s+NAE_STRETCH_TRANSIENTS\s+4u\b", h)
    later = h[h.index("Later additions within 3"):h.index("*/", h.index("Later additions within 3"))]
    assert "NAE_STRETCH_TRANSIENTS" in later
    assert re.search(r"#define\s+NAE_ABI_VERSION\s+3\b", h)
    assert nae.STRETCH_TRANSIENTS == 4
    spec = open(os.path.join(ROOT, "include", "nae_dsp_spec.h")).read()
    for name in ("NAE_TRANSIENT_RISE", "NAE_TRANSIENT_FLOOR", "NAE_TRANSIENT_NUM", "NAE_TRANSIENT_DEN"):
        assert re.search(r"#define\s+" + name + r"\s", spec), name


def test_host_node_transients_key(tmp_path):
    """Velocity_modifier / Pitch_modifier: "transients" is absent by default, written back only when true, a non-bool or true with
    "phase_lock" is "Wrong field: transients", it combines with "fft_size" and "formant" and is kept with the soundtouch algorithm"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "json", "transients"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST PV NODE OK json transients" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
