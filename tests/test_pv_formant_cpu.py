"""Formant preservation ("Formant preservation"), no GPU: the CPU statement tests/pv_formant/ref_pv_formant.c pinned to the
vocoder statements at lifter 0 and to the float64 numpy statement (tests/pv_formant_numpy.py) with a lifter, what it does to a vowel, the
default lifter, the C ABI's declarations and the host node's "formant" key."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import pv_formant_numpy
import pv_formant_ref
import pv_lock_ref
import pv_sizes_ref
from conftest import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nae_stretch_formant_lifter", "nae_stretch_block_formant_f32", "nae_stretch_create_formant")
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5), (0.5, 2.0), (2.0, 1.0)]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ref_pv_formant"))
    return pv_formant_ref.build(d), pv_sizes_ref.build(d), pv_lock_ref.build(d)


def tone(L, f=(1000.0, 3300.0), amp=(0.5, 0.25)):
    n = np.arange(L)
    return sum(a * np.sin(2 * np.pi * fr * n / 48000) for a, fr in zip(amp, f)).astype(np.float32)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", PAIRS)
def test_lifter_zero_is_the_vocoder_statements(refs, rate, pitch, ch):
    """lifter 0: ref_pv_sizes.c bit for bit at every size, and ref_pv_lock.c bit for bit when locked"""
    F, S, K = refs
    L = 20000
    m = tone(L)
    for x in (orc.fill_uniform(L * ch, 3), np.stack([m, 0.5 * m], 1).reshape(-1) if ch == 2 else m):
        for n_fft in pv_formant_ref.SIZES:
            a, b = pv_formant_ref.stretch(F, x, ch, rate, pitch, n_fft, 0), pv_sizes_ref.stretch(S, x, ch, rate, pitch, n_fft)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n_fft
        a, b = pv_formant_ref.stretch(F, x, ch, rate, pitch, 1024, 0, lock=True), pv_lock_ref.stretch(K, x, ch, rate, pitch, True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "locked"


@pytest.mark.parametrize("n_fft", pv_formant_ref.SIZES)
@pytest.mark.parametrize("rate,pitch", [(1.0, 2.0), (0.25, 2.0)])
def test_statement_matches_the_numpy_specification(refs, n_fft, rate, pitch):
    """tempo 1/2 in both stage orders (rho = 2: transposer first; rho = 1/2: vocoder first), default lifter, white noise: within 1e-5 of the
    float64 statement (measured 4.1e-7 - 5.3e-7).  The signal has energy in every bin on purpose: in a bin that float64 leaves near zero the
    float32 transform leaves its rounding noise (~1e-7 of the frame), and the log spectrum, hence the envelope, follows that floor — the
    two-tone signal of tests/test_pv_sizes_cpu.py differs by 1e-5 - 1.5e-3 here for that reason alone."""
    F = refs[0]
    x = orc.fill_uniform(24000, 3)
    q = pv_formant_ref.default_lifter(48000, n_fft)
    got = pv_formant_ref.stretch(F, x, 1, rate, pitch, n_fft, q)
    want = pv_formant_numpy.stretch(x, 1, rate, pitch, n_fft, q)
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
def test_vowel_keeps_its_envelope(refs, n_fft, semitones):
    """a 140 Hz vowel at 48 kHz (F1 centroid 717 Hz in), pitch +4 / -5 semitones.  Measured with the default lifter: RMS error 2.1 - 4.4 dB,
    F1 centroid 733 - 773 Hz (+16 ... +56); unflagged: 10.5 - 11.0 dB, F1 834 Hz (+4) and 635 - 642 Hz (-5), i.e. +117 / -82 Hz.  Bars: 6 dB
    and 65 Hz."""
    F = refs[0]
    x = vowel(48000)
    e_in, f1_in = harmonic_quality(x, F0)
    assert e_in < 0.01 and abs(f1_in - 717) < 5
    p = 2 ** (semitones / 12)
    q = pv_formant_ref.default_lifter(SR, n_fft)
    e_on, f1_on = harmonic_quality(pv_formant_ref.stretch(F, x, 1, 1.0, p, n_fft, q), F0 * p)
    e_off, f1_off = harmonic_quality(pv_formant_ref.stretch(F, x, 1, 1.0, p, n_fft, 0), F0 * p)
    print(f"N={n_fft} {semitones:+d}: formant {e_on:.2f} dB F1 {f1_on:.0f} Hz; unflagged {e_off:.2f} dB F1 {f1_off:.0f} Hz")
    assert e_on <= 6.0 and abs(f1_on - f1_in) <= 65
    assert e_off > 6.0 and abs(f1_off - f1_in) > 65


def test_default_lifter(nae):
    for sr, want in ((8000, 11), (44100, 63), (48000, 68)):
        for n_fft in pv_formant_ref.SIZES:
            w = min(want, n_fft // 4)
            assert nae.formant_lifter(sr, n_fft) == w == pv_formant_ref.default_lifter(sr, n_fft), (sr, n_fft)
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


def build_host_pv_formant(out_dir):
    """tests/pv_formant/host_pv_formant.cpp with the flags of tests/host/Makefile"""
    pkg = os.path.join(ROOT, "nodey-audio-editor_amd")
    for d in (pkg, os.path.join(pkg, "host")):
        r = subprocess.run(["make", "-C", d, "-j4"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exe = os.path.join(out_dir, "host_pv_formant")
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-pthread", "-Wall", "-Wno-unused-parameter", "-I" + os.path.join(pkg, "host"),
           "-I" + os.path.join(ROOT, "include"), "-ffp-contract=off", os.path.join(ROOT, "tests", "pv_formant", "host_pv_formant.cpp"), "-o", exe,
           os.path.join(pkg, "host", "libnae_host.a"), "-L" + pkg, "-lnae_gpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_node_formant_key(tmp_path):
    """Pitch_modifier: "formant" round-trips, is absent by default and when false, a value that is not a bool is "Wrong field: formant", it
    combines with phase_lock and fft_size, is kept with the soundtouch algorithm; Velocity_modifier has no such key"""
    exe = build_host_pv_formant(str(tmp_path))
    r = subprocess.run([exe, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST PV FORMANT OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
