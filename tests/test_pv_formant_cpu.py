"""Formant preservation ("Formant preservation"), no GPU: the CPU statement tests/pv_ref/ref_pv.c pinned at lifter 0 to the
oracle and to the recorded integer phases of every other size and of the phase lock (tests/golden/pv_synth_phase.json), and with a lifter to
the float64 numpy statement (tests/pv_sizes_numpy.py); what it does to a vowel, the default lifter, the C ABI's declarations and the host
node's "formant" key."""
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
import pv_sizes_numpy
from conftest import rel_rms
from pv_gpu import tone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nae_stretch_formant_lifter", "nae_stretch_block_formant_f32", "nae_stretch_create_formant")
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5), (0.5, 2.0), (2.0, 1.0)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def phase_digest(qs):
    return hashlib.sha256(np.ascontiguousarray(qs, "<i4").tobytes()).hexdigest()


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", PAIRS)
def test_lifter_zero_is_the_vocoder_statements(ref, rate, pitch, ch):
    """lifter 0: the oracle bit for bit at 1024 unlocked; the integer synthesis phases at 512 / 2048 / 4096 and locked at 1024 are those
    recorded in tests/golden/pv_synth_phase.json (sha256 of the int32 [frames][ch][N/2 + 1] array) from the two statements this one
    replaced, at commit 9447921; without the vocoder (2.0, 1.0) every size and the lock give the oracle's samples"""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pv_synth_phase.json")))
    L = 20000
    m = tone(L)
    pv_on = orc.plan(rate, pitch, L)[1].pv_on
    for kind, x in (("noise", orc.fill_uniform(L * ch, 3)), ("tone", np.stack([m, 0.5 * m], 1).reshape(-1) if ch == 2 else m)):
        want = orc.stretch(x, ch, rate, pitch)
        assert np.array_equal(pv_ref.stretch(ref, x, ch, rate, pitch, 1024, lifter=0).view(np.uint32), want.view(np.uint32)), kind
        for n_fft, lock in ((512, False), (2048, False), (4096, False), (1024, True)):
            if pv_on:
                key = f"{rate!r} {pitch!r} ch{ch} {kind} {n_fft}" + (" locked" if lock else "")
                assert phase_digest(pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock)) == golden[key], key
            else:
                got = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, n_fft, lock)


@pytest.mark.parametrize("n_fft", pv_ref.SIZES)
@pytest.mark.parametrize("rate,pitch", [(1.0, 2.0), (0.25, 2.0)])
def test_statement_matches_the_numpy_specification(ref, n_fft, rate, pitch):
    """tempo 1/2 in both stage orders (rho = 2: transposer first; rho = 1/2: vocoder first), default lifter, white noise: within 1e-5 of the
    float64 statement (measured 4.1e-7 - 5.3e-7).  The signal has energy in every bin on purpose: in a bin that float64 leaves near zero the
    float32 transform leaves its rounding noise (~1e-7 of the frame), and the log spectrum, hence the envelope, follows that floor — the
    two-tone signal of tests/test_pv_sizes_cpu.py differs by 1e-5 - 1.5e-3 here for that reason alone."""
    x = orc.fill_uniform(24000, 3)
    q = pv_ref.default_lifter(48000, n_fft)
    got = pv_ref.stretch(ref, x, 1, rate, pitch, n_fft, lifter=q)
    want = pv_sizes_numpy.stretch(x, 1, rate, pitch, n_fft, q)
    assert got.size == want.size
    assert rel_rms(got, want) <= 1e-5, rel_rms(got, want)


SR, F0 = 48000, 140.0


def envelope(f):
    """the vowel's spectral envelope: resonances at 700, 1200 and 2600 Hz over a floor"""
    return 0.03 + np.exp(-0.5 * ((f - 700) / 130) ** 2) + 0.6 * np.exp(-0.5 * ((f - 1200) / 150) ** 2) + 0.3 * np.exp(-0.5 * ((f - 2600) / 220) ** 2)


def vowel(L):
    t = np.arange(L) / SR
    y = np.zeros(L)
    for h in range(1, int(8000 / F0)):
        y += envelope(h * F0) * np.sin(2 * np.pi * h * F0 * t + 0.7 * h * h)
    return (0.1 * y).astype(np.float32)


def harmonic_quality(y, f0):
    """(RMS dB error of the harmonic amplitudes below 5 kHz against the input envelope after removing the mean, F1 estimate): amplitudes from a
    Hann DFT of the steady middle half; F1 = the power centroid of the harmonics in 350 - 1050 Hz"""
    mid = y[y.size // 4: 3 * y.size // 4].astype(np.float64)
    w = np.hanning(mid.size)
    t = np.arange(mid.size) / SR
    f = np.arange(1, int(5000 / f0) + 1) * f0
    a = np.array([abs(np.sum(mid * w * np.exp(-2j * np.pi * fr * t))) for fr in f])
    err = 20 * np.log10(a) - 20 * np.log10(envelope(f))
    err -= err.mean()
    sel = (f >= 350) & (f <= 1050)
    return float(np.sqrt(np.mean(err ** 2))), float(np.sum(f[sel] * a[sel] ** 2) / np.sum(a[sel] ** 2))


@pytest.mark.parametrize("semitones", [4, -5])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_vowel_keeps_its_envelope(ref, n_fft, semitones):
    """a 140 Hz vowel at 48 kHz (F1 centroid 717 Hz in), pitch +4 / -5 semitones.  Measured with the default lifter: RMS error 2.1 - 4.4 dB,
    F1 centroid 733 - 773 Hz (+16 ... +56); unflagged: 10.5 - 11.0 dB, F1 834 Hz (+4) and 635 - 642 Hz (-5), i.e. +117 / -82 Hz.  Bars: 6 dB
    and 65 Hz."""
    x = vowel(48000)
    e_in, f1_in = harmonic_quality(x, F0)
    assert e_in < 0.01 and abs(f1_in - 717) < 5
    p = 2 ** (semitones / 12)
    q = pv_ref.default_lifter(SR, n_fft)
    e_on, f1_on = harmonic_quality(pv_ref.stretch(ref, x, 1, 1.0, p, n_fft, lifter=q), F0 * p)
    e_off, f1_off = harmonic_quality(pv_ref.stretch(ref, x, 1, 1.0, p, n_fft, lifter=0), F0 * p)
    print(f"N={n_fft} {semitones:+d}: formant {e_on:.2f} dB F1 {f1_on:.0f} Hz; unflagged {e_off:.2f} dB F1 {f1_off:.0f} Hz")
    assert e_on <= 6.0 and abs(f1_on - f1_in) <= 65
    assert e_off > 6.0 and abs(f1_off - f1_in) > 65


def test_default_lifter(nae):
    for sr, want in ((8000, 11), (44100, 63), (48000, 68)):
        for n_fft in pv_ref.SIZES:
            w = min(want, n_fft // 4)
            assert nae.formant_lifter(sr, n_fft) == w == pv_ref.default_lifter(sr, n_fft), (sr, n_fft)
    for n_fft in (256, 1000, 8192, 0):
        assert nae.formant_lifter(48000, n_fft) == 0
    assert nae.formant_lifter(0, 1024) == 0 and nae.formant_lifter(300, 1024) == 1


def test_abi_declares_the_formant_entries(nae):
    hdr = open(os.path.join(ROOT, "include", "nae_gpu.h")).read()
    assert re.search(r"#define NAE_ABI_VERSION 3\b", hdr)
    later = hdr[hdr.index("Later additions within 3"): hdr.index("#define NAE_ABI_VERSION")]
    spec = open(os.path.join(ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define NAE_FORMANT_MAX_GAIN 16\.0f\b", spec)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in later, s
        assert s in nae.EXPORTED_SYMBOLS, s
        assert hasattr(nae.load_library(), s), s


def test_host_node_formant_key(tmp_path):
    """Pitch_modifier: "formant" round-trips, is absent by default and when false, a value that is not a bool is "Wrong field: formant", it
    combines with phase_lock and fft_size, is kept with the soundtouch algorithm; Velocity_modifier has no such key"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "json", "formant"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST PV NODE OK json formant" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
