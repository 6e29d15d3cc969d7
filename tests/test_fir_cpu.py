"""K9 FIR filter, no GPU: the CPU statement (tests/fir_ref/ref_fir.c) against a float64 direct convolution at every frame size; the library's
host-side entries nae_fir_design and nae_fir_pick_n_fft against their restatements (tests/fir_ref.py); the host node's JSON keys and the
two registration calls (tests/fir_ref/host_fir_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fir_ref
import node_harness
from conftest import rel_rms

# the statement against float64: the bound the project uses for its float64 pins.  Measured 1.3e-7 ... 3.4e-7 ("K9 FIR filter")
RMS_BOUND = 1e-5


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return fir_ref.build(str(tmp_path_factory.mktemp("ref_fir")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("fir_ref/host_fir_node.cpp", str(tmp_path_factory.mktemp("host_fir")))


def _signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return {"noise": rng.uniform(-1, 1, n).astype(np.float32),
            "two-tone": (0.6 * np.sin(2 * np.pi * 0.0371 * t) + 0.3 * np.sin(2 * np.pi * 0.213 * t + 1.0)).astype(np.float32)}


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_statement_against_float64_convolution(ref, n_fft):
    B = n_fft // 2
    in_len = 3 * B + 7
    rng = np.random.default_rng(100 + n_fft)
    for L in (1, 2, 65, B + 1):
        taps = rng.uniform(-1, 1, L).astype(np.float32)
        for name, x in _signals(in_len, n_fft + L).items():
            got = fir_ref.run(ref, taps, n_fft, x)
            want = fir_ref.direct(taps, x)
            err = rel_rms(got, want)
            print(f"n_fft {n_fft} L {L} {name}: rel RMS {err:.2e}")
            assert err <= RMS_BOUND, (n_fft, L, name, err)


def test_statement_is_causal_and_stereo_channels_are_independent(ref):
    """an impulse at sample p gives the taps from p on; the interleaved form filters each channel by itself"""
    taps = np.arange(1, 8, dtype=np.float32)
    x = np.zeros(700, np.float32)
    x[300] = 1.0
    y = fir_ref.run(ref, taps, 512, x)
    assert np.allclose(y[300:307], taps, atol=1e-5) and np.abs(y[:300]).max() < 1e-5 and np.abs(y[307:]).max() < 1e-5
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, 700).astype(np.float32), rng.uniform(-1, 1, 700).astype(np.float32)
    st = fir_ref.run(ref, taps, 512, np.stack([a, b], 1).reshape(-1), ch=2).reshape(-1, 2)
    assert np.array_equal(st[:, 0].view(np.uint32), fir_ref.run(ref, taps, 512, a).view(np.uint32))
    assert np.array_equal(st[:, 1].view(np.uint32), fir_ref.run(ref, taps, 512, b).view(np.uint32))


def test_statement_rejects_what_the_specification_excludes(ref):
    x = np.zeros(16, np.float32)
    y = np.zeros(16, np.float32)
    h = np.zeros(4096, np.float32)
    for L, n in ((0, 512), (258, 512), (1, 256), (1, 1000), (2050, 4096), (1, 8192)):
        assert ref.ref_fir_run(h.ctypes.data, L, n, x.ctypes.data, 16, 1, y.ctypes.data) == -1, (L, n)


def test_pick_n_fft(nae, ref):
    lib = nae.load_library()
    for L in range(1, 2051):
        want = 512 if L <= 257 else 1024 if L <= 513 else 2048 if L <= 1025 else 4096 if L <= 2049 else 0
        assert lib.nae_fir_pick_n_fft(L) == want == fir_ref.pick_n_fft(L) == ref.ref_fir_pick_n_fft(L), L
        assert nae.Context.fir_pick_n_fft(L) == want
    for L in (0, -1, -2049, 1 << 30):
        assert lib.nae_fir_pick_n_fft(L) == 0, L


def _ulp_diff(a, b):
    """distance in f32 units in the last place (of the larger magnitude's binade), elementwise"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a64 - b64) / ulp


@pytest.mark.parametrize("sample_rate", (44100, 48000))
@pytest.mark.parametrize("kind", fir_ref.KINDS)
def test_design_against_float64_restatement(nae, kind, sample_rate):
    """at most one f32 unit in the last place per tap: both sides round the same double formula once; libm's sin is the only difference"""
    for L, f_lo, f_hi in ((513, 300.0, 1000.0), (65, 2000.0, 9000.5), (1, 100.0, 200.0), (2049, 40.0, 19000.0), (3, 5000.0, 5001.0)):
        got = nae.Context.fir_design(kind, sample_rate, f_lo, f_hi, L)
        want = fir_ref.design(kind, sample_rate, f_lo, f_hi, L).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (L,)
        d = _ulp_diff(got, want)
        print(f"{kind} {sample_rate} L {L}: max {d.max():.1f} ulp, {int((d > 0).sum())} taps differ")
        assert d.max() <= 1.0, (kind, sample_rate, L, d.max())
        assert np.array_equal(got, got[::-1]), "type-I linear phase: symmetric taps"


def _response_db(taps, f, sample_rate):
    n = 1 << 18
    H = np.abs(np.fft.rfft(taps.astype(np.float64), n))
    return 20.0 * np.log10(max(H[int(round(f / sample_rate * n))], 1e-300))


def test_designed_lowpass_response(nae):
    """L = 513, 1 kHz at 48 kHz: within 0.1 dB of 0 dB at half the cutoff, below -60 dB at twice the cutoff (Kaiser 8: the transition band
    is about 480 Hz wide around the cutoff and the stop band lies near -80 dB)"""
    taps = nae.Context.fir_design("lowpass", 48000, 0.0, 1000.0, 513)
    p, s = _response_db(taps, 500.0, 48000), _response_db(taps, 2000.0, 48000)
    print(f"lowpass 1 kHz / 513 taps: {p:+.4f} dB at 500 Hz, {s:.1f} dB at 2 kHz, sum {taps.astype(np.float64).sum():.9f}")
    assert abs(p) <= 0.1 and s < -60.0
    assert abs(taps.astype(np.float64).sum() - 1.0) < 1e-6          # sum h = 1 before rounding
    # the complements: a high-pass removes DC, a band-stop keeps it
    for kind, dc in (("highpass", 0.0), ("bandpass", 0.0), ("bandstop", 1.0)):
        h = nae.Context.fir_design(kind, 48000, 1000.0, 4000.0, 513)
        assert abs(h.astype(np.float64).sum() - dc) < 1e-6, kind


def test_design_rejections(nae):
    lib = nae.load_library()
    out = np.zeros(4096, np.float32)
    d = lambda kind, sr, lo, hi, L, p=out.ctypes.data: lib.nae_fir_design(kind, sr, lo, hi, L, p)
    assert d(0, 48000, 0.0, 1000.0, 513) == 0 and d(1, 48000, 1000.0, 0.0, 513) == 0      # the unused frequency is ignored
    assert d(2, 48000, 100.0, 1000.0, 513) == 0 and d(3, 48000, 100.0, 1000.0, 513) == 0
    nan = float("nan")
    for args in ((0, 48000, 0.0, 0.0, 513), (0, 48000, 0.0, 24000.0, 513), (0, 48000, 0.0, -5.0, 513), (0, 48000, 0.0, nan, 513),
                 (1, 48000, 0.0, 1000.0, 513), (1, 48000, 24000.0, 1000.0, 513), (1, 48000, nan, 1000.0, 513),
                 (2, 48000, 1000.0, 1000.0, 513), (2, 48000, 2000.0, 1000.0, 513), (2, 48000, 0.0, 1000.0, 513), (2, 48000, 100.0, 24000.0, 513),
                 (3, 48000, 2000.0, 1000.0, 513), (3, 44100, 100.0, 22050.0, 513),
                 (0, 48000, 0.0, 1000.0, 512), (0, 48000, 0.0, 1000.0, 0), (0, 48000, 0.0, 1000.0, -3),
                 (4, 48000, 100.0, 1000.0, 513), (-1, 48000, 100.0, 1000.0, 513), (0, 0, 0.0, 1000.0, 513), (0, -48000, 0.0, 1000.0, 513)):
        assert d(*args) == -1, args
    assert d(0, 48000, 0.0, 1000.0, 513, None) == -1
    with pytest.raises(nae.NaeError):
        nae.Context.fir_design("lowpass", 48000, 0.0, 30000.0, 513)


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type is "Wrong field: <key>" """
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST FIR OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """register_all_processors() alone leaves the mirror of the reference's list at 7 entries; register_extension_processors() adds
    audio_filter as the eighth"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST FIR OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert len(lines) == 2 and len(lines[0]) == 7 and "audio_filter" not in lines[0]
    assert len(lines[1]) == 8 and sorted(lines[1]) == sorted(lines[0] + ["audio_filter"])
